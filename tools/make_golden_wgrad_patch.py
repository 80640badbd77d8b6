"""Records what the range-patch weight gradient computed BEFORE its stage ring, for tests/test_wgrad_patch_ring_gpu.py.

    python tools/make_golden_wgrad_patch.py [--out FILE]     -> tests/golden/wgrad_patch_parent.json

Run once on the MI355X with the library of the commit before the ring (this file and tests/wgrad_patch_ring_cases.py copied into its
tree); never recomputed from the code under test.  For every case of tests.wgrad_patch_ring_cases.CASES (seeded N(0,1) operands): the
split count and the SHA-256 of the partial slabs `part` and of the reduced gradient.  Every case is run twice and must give the same bits
before anything is written.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wgrad_patch_ring_cases as W  # noqa: E402


def digest(kind, shape):
    r = W.run(kind, shape)
    return {"nsplit": r["nsplit"], "part": W.sha(r["part"]), "grad": W.sha(r["grad"])}


def main(out):
    rec = {}
    for kind, shape in W.CASES:
        first, second = digest(kind, shape), digest(kind, shape)
        assert first == second, (kind, shape, first, second)
        rec[W.case_id(kind, shape)] = first
        print(W.case_id(kind, shape), first, flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("->", out)


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden", "wgrad_patch_parent.json"))
