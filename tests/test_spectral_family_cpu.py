"""The spectral-norm kernels without a GPU: the closed-form weight gradient of tests/spectral_ref64.py against float64 autograd of
torch.nn.utils.spectral_norm's own step, the regimes the tables of tests/spectral_cases.py name, the emulator's statement inside the
derived bounds -- which therefore admit an honest fp32 implementation -- and every deliberately wrong reference outside them.
tests/test_spectral_family_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx
from tests import spectral_cases as P
from tests import spectral_ref64 as R
from tests.emulator_dfamily import DFamilyEmuOps


def make():
    return Ctx(DFamilyEmuOps(), "cpu", BF16)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 40), (40, 40)])
@pytest.mark.parametrize("power_iter", [True, False])
def test_closed_form_gradient_equals_float64_autograd(h, w, power_iter):
    g = torch.Generator().manual_seed(h * 100 + w)
    W, G = torch.randn(h, w, generator=g, dtype=torch.float64) * 0.05, torch.randn(h, w, generator=g, dtype=torch.float64)
    u0 = torch.nn.functional.normalize(torch.randn(h, generator=g, dtype=torch.float64), dim=0)
    v0 = torch.nn.functional.normalize(torch.randn(w, generator=g, dtype=torch.float64), dim=0)
    u, v, sigma, dW = R.module_step64(W, u0, v0, G, power_iter)
    tol = dict(rtol=1e-12, atol=1e-12)
    if power_iter:
        v1 = R.v64(W, u0, v0, 1e-12)
        u1 = R.u64(W, v1, 1e-12)
        torch.testing.assert_close(v1, v, **tol)
        torch.testing.assert_close(u1, u, **tol)
    s = R.sigma64(W, u0, u, v)
    assert abs(s - float(sigma)) <= 1e-12 * abs(s)
    torch.testing.assert_close(R.dW64(G, R.gw64(G, W) / s, u, v, s), dW, **tol)
    torch.testing.assert_close(R.dW64(G, R.gw64(G, W / s), u, v, s), dW, **tol)          # the single-matrix path's <G, W_sn>


def test_every_table_is_in_its_regime():
    for c in P.CASES:
        P.check_regime(c)
    assert len({c.name for c in P.CASES}) == len(P.CASES) and len(P.WRONG) >= 10
    assert all(n in P.BY_NAME for _, names in P.WRONG for n in names)
    assert {len(P.TABLES[k]) for k in ("t1", "t2", "t3", "t16", "t17")} == {1, 2, 3, 16, 17}
    assert len(P.PAIRS) <= 12 and {h for h, _ in P.PAIRS} == {1, 31, 32, 33, 64} and {w for _, w in P.PAIRS} == {1, 255, 256, 257, 300}


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_emulated_family_within_the_derived_bounds(c):
    P.body(make, c)


@pytest.mark.parametrize("where", ["W", "u", "G"])
def test_emulated_nan_stays_in_its_descriptor(where):
    P.body_nonfinite(make, where)


@pytest.mark.parametrize("where", ["W", "u", "v", "G"])
def test_emulated_nan_single_matrix_path(where):
    P.body_nonfinite_single(make, where)


@pytest.mark.parametrize("wrong,names", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_emulated_family_rejects_a_wrong_reference(wrong, names):
    P.rejects(make, wrong, names)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in P.CASES:          # run alone, this test fills the table itself (results are cached per case)
        P.body(make, c)
    worst = P.worst_table(False)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
