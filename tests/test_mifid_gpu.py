"""The evaluation kernels of csrc/mifid.hip on the GPU through HipOps, and gan_variant_research_amd.evaluate on top of them: the bodies of
tests/mifid_cases.py (tests/test_mifid_cpu.py runs the same bodies on the emulator), element by element against the long-double and
float64 statements of tests/mifid_ref64.py with the derived bounds.

What the cases reach: every extent from {1, 15, 16, 17, 63, 65, 130} on both sides of the 64 x 64 tile and the 16-wide MFMA tile,
contraction lengths around the step of 4 and the slab of 16 and one of 2049, both operand walks, float32 and float64 inputs mixed,
row strides above the column count, null and non-null centres and scales, A is B, sentinels past every output extent, the same bits
from a repeated call, the f64 accumulator map (identity against an asymmetric matrix), the row minimum's planted minima, ties and
left-out rows and columns, the moments at a common offset of 1e6, and the metric end to end."""
import pytest
import torch

from gan_variant_research_amd.runtime import HipOps
from tests import mifid_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return HipOps(torch.device(DEV)), DEV


@pytest.mark.parametrize("r", N.GRAM_RUNS, ids=N.run_id)
def test_contraction_within_the_derived_bound(r):
    N.body_gram(make, r)


def test_contraction_orientation():
    N.body_gram_orientation(make)


@pytest.mark.parametrize("r", N.MOMENT_RUNS, ids=N.run_id)
def test_moments_within_the_derived_bounds(r):
    N.body_moments(make, r)


def test_moments_flag_nan_and_inf():
    N.body_moments_flag(make)


@pytest.mark.parametrize("r", N.ROWMIN_RUNS, ids=N.run_id)
def test_row_minimum(r):
    N.body_rowmin(make, r)


def test_row_minimum_with_nothing_left():
    N.body_rowmin_nothing_left(make)


def test_entries_refuse_bad_arguments():
    N.body_refused(make)


@pytest.mark.parametrize("shape", N.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metric_against_float64(shape):
    N.body_metric(make, shape)


def test_identical_sets_give_zero():
    N.body_identical_sets(make)


@pytest.mark.parametrize("shape", N.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_cosine_analysis(shape):
    N.body_cosine(make, shape)


def test_refusals_name_their_cause():
    N.body_refusals(make)


def test_wrong_references_are_rejected():
    N.body_wrong_references(make)


def test_metric_equals_the_reference_recorded_results():
    N.body_golden_metric(make)


def test_cache_files_load_on_either_side(tmp_path):
    N.body_cache(make, tmp_path)
