"""With loss_weights.featmatch 0 or absent, cut.CutTrainer builds launch for launch the step programs of the commit before the key was read:
the same entry points in the same order in every program of both step shapes, the same scalars, view geometries and tensor sizes, the same
`losses` size and the same loss-dict keys (tools/make_golden_featmatch_parent.py lists the cases and what a record holds)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_featmatch_parent as M  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(M.GOLDEN) as f:
        return json.load(f)


def test_every_case_of_the_tool_is_in_the_golden_file(golden):
    assert sorted(golden["cases"]) == sorted(M.CASES) and len(M.CASES) == 8
    for name in M.CASES:
        rec = M.unpack(golden, name)
        assert "featmatch" not in rec["keys"] and rec["keys"] == M.unpack(golden, "absent-k1")["keys"]
        assert rec == M.unpack(golden, name.replace("zero", "absent")), name
        names = [l[0] for l in rec["programs"]["merged=True"]["prog_g_adversarial"]]
        assert "featmatch" not in names and names.count("patch_loss") == M.CASES[name][1]


@pytest.mark.parametrize("name", list(M.CASES))
def test_builds_the_parents_launches(golden, name):
    """tests/golden/featmatch_parent_launches.json was recorded ON the parent commit by tools/make_golden_featmatch_parent.py (copied into
    its tree); it is not recomputed from the code under test."""
    want, got = M.unpack(golden, name), M.record(name)
    assert got["losses"] == want["losses"] and got["keys"] == want["keys"]
    for mode, progs in want["programs"].items():
        for p, launches in progs.items():
            g = got["programs"][mode][p]
            assert (g is None) == (launches is None), (mode, p)
            if launches is None:
                continue
            assert [l[0] for l in g] == [l[0] for l in launches], (mode, p)
            for i, (a, b) in enumerate(zip(g, launches)):
                assert a == b, (mode, p, i, a, b)
