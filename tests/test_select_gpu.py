"""The selection entries of csrc/mifid.hip (gan_sqdist_rowmin, gan_kmeans_update) on the GPU through HipOps, element by element against
the long-double statements of tests/select_ref64.py with the bounds of tests/select_cases.py, and gan_variant_research_amd.select_7k on
top of them: the same labels and the same chosen order as on the emulator.

What the cases reach: (M, N, K) of (1, 1, 1), (65, 129, 17), (70, 130, 2048) and (300, 128, 2048); float32 and float64 operands mixed;
row strides above the column count; the transform on one side only and on both; a zero-variance column; a row bit-identical to a centre;
two identical centres on both sides of the 64-column tile; k = 1, one cluster holding every row, D = 1 and D = 33 and 257, more rows
than one 256-row chunk, labels out of range; sentinels past every output and the workspace; the same bits from a repeated call."""
import numpy as np
import pytest
import torch

from gan_variant_research_amd import select_7k as S
from gan_variant_research_amd.runtime import HipOps
from tests import select_cases as N
from tests.emulator_select import SelectEmuOps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return HipOps(torch.device(DEV)), DEV


@pytest.mark.parametrize("r", N.SQ_RUNS, ids=N.sq_id)
def test_sqdist_rowmin_within_the_bound(r):
    N.body_sqdist(make, r)


def test_sqdist_rowmin_tie_goes_to_the_lower_tile():
    N.body_sqdist_tie_across_tiles(make)


def test_sqdist_rowmin_refuses_bad_arguments():
    N.body_sqdist_refused(make)


@pytest.mark.parametrize("r", N.KU_RUNS, ids=N.ku_id)
def test_kmeans_update_within_the_bound(r):
    N.body_kmeans_update(make, r)


def test_kmeans_update_refuses_bad_arguments():
    N.body_kmeans_update_refused(make)


def test_kmeans_fit_gives_the_emulator_labels():
    x, k = N.KM_FIXTURES["gauss97x33"]()
    got = S.kmeans_fit(x, k, device=DEV)
    emu = S.kmeans_fit(x, k, device="cpu", ops=SelectEmuOps())
    assert np.array_equal(got["labels"], emu["labels"]) and got["n_iter"] == emu["n_iter"]
    assert np.abs(got["centers"] - emu["centers"]).max() <= 1e-12 and abs(got["inertia"] - emu["inertia"]) <= 1e-12 * emu["inertia"]
    N.body_kmeans_fixture(make, "gauss97x33")


def test_kmeans_fit_at_the_selection_shape_equals_scikit_learn():
    N.body_kmeans_fixture(make, "relu300x2048")          # 300 x 2048, k = 128: the shape the selection runs


def test_kmeans_fit_relocates_an_empty_cluster():
    N.body_kmeans_empty_cluster(make)


def test_select_gives_the_emulator_order():
    got = N.body_select(make)
    real, cands = N.select_fixture()
    emu = S.select(real, cands, tau=0.22, k=16, target=200, device="cpu", ops=SelectEmuOps(), verbose=False)
    assert np.array_equal(got["chosen"], emu["chosen"]) and np.array_equal(got["kmeans"]["labels"], emu["kmeans"]["labels"])
