"""The library reads exactly these environment variables.  Every "GAN_..." string literal in the package's Python and HIP sources is
one of them, so a new run-time switch (an A/B knob, a diagnostic) cannot land without this list changing with it."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gan-variant-research_amd")

KEPT = {
    "GAN_PATCH_BM",        # range-patch tile rows / columns, forced at planning time (the GPU tests reach the 288-row and 256-channel tiles)
    "GAN_PATCH_BN",
    "GAN_SINGLE_STREAM",   # one HIP stream: the bit-equality test and the profiling tools
    "GAN_NO_BWD_CHAIN",    # chained against unchained backward (test_engine_cpu.py)
    "GAN_NO_BUCKET_AR",    # one all-reduce instead of two buckets (the one-rank RCCL test)
    "GAN_DEBUG_SYNC",      # names and synchronises every launch (fault attribution)
}


def _sources():
    files = glob.glob(os.path.join(PKG, "*.py"))
    files += glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))
    return sorted(files)


def test_environment_variables_are_the_kept_set():
    found = {}
    for path in _sources():
        with open(path, encoding="utf-8") as f:
            for m in re.finditer(r"""(["'])(GAN_[A-Z0-9_]*)\1""", f.read()):
                found.setdefault(m.group(2), []).append(os.path.relpath(path, ROOT))
    assert set(found) == KEPT, {k: v for k, v in found.items() if k not in KEPT} or sorted(KEPT - set(found))
