"""gan_variant_research_amd.evaluate and the entries of csrc/mifid.hip without a GPU: the bodies of tests/mifid_cases.py on the emulator of
tests/emulator_mifid.py, held to the float64 / long-double statements of tests/mifid_ref64.py with the derived bounds, and to the
reference's recorded results under tests/golden/.  tests/test_mifid_gpu.py runs the same bodies on the HIP kernels."""
import pytest

from tests import mifid_cases as N
from tests.emulator_mifid import MifidEmuOps


def make():
    return MifidEmuOps(), "cpu"


def test_run_list_covers_the_edges():
    t0 = [r for r in N.GRAM_RUNS if r.trans == 0]
    t1 = [r for r in N.GRAM_RUNS if r.trans == 1]
    assert {r.M for r in t0} >= {1, 15, 16, 17, 63, 65, 130} and {r.N for r in t0} >= {1, 15, 16, 17, 63, 65, 130}
    assert {r.K for r in t0} >= {1, 3, 4, 5, 40, 130, 2049}
    assert {r.K for r in t1} == {2, 5, 33, 257} and {r.M for r in t1} == {1, 17, 64, 130}
    for runs in (t0, t1):
        assert {r.da for r in runs} == {r.db for r in runs} == {"f32", "f64"}
        assert {r.pad > 0 for r in runs} == {True, False} and {r.centre for r in runs} == {True, False} and {r.same for r in runs} == {True, False}
    assert {r.scale for r in t0} == {True, False}
    assert len(set(N.GRAM_RUNS)) == len(N.GRAM_RUNS)


@pytest.mark.parametrize("r", N.GRAM_RUNS, ids=N.run_id)
def test_emulated_contraction_within_the_derived_bound(r):
    N.body_gram(make, r)


def test_emulated_contraction_orientation():
    N.body_gram_orientation(make)


@pytest.mark.parametrize("r", N.MOMENT_RUNS, ids=N.run_id)
def test_emulated_moments_within_the_derived_bounds(r):
    N.body_moments(make, r)


def test_emulated_moments_flag_nan_and_inf():
    N.body_moments_flag(make)


@pytest.mark.parametrize("r", N.ROWMIN_RUNS, ids=N.run_id)
def test_emulated_row_minimum(r):
    N.body_rowmin(make, r)


def test_emulated_row_minimum_with_nothing_left():
    N.body_rowmin_nothing_left(make)


def test_emulated_entries_refuse_bad_arguments():
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


def test_folder_helpers_and_report_equal_the_reference_recorded_results(tmp_path):
    N.body_golden_files(tmp_path)


def test_cache_files_load_on_either_side(tmp_path):
    N.body_cache(make, tmp_path)


def test_command_line_without_an_extractor_names_the_three_flags(tmp_path, monkeypatch):
    """Where torchmetrics does not import, the command ends with one sentence that names --extractor, --real-features and --fake-features; TFDS
    mode is refused as the reference's CLI refuses it."""
    import sys
    from gan_variant_research_amd import evaluate as E
    monkeypatch.setitem(sys.modules, "torchmetrics.image.fid", None)          # the import fails here, wherever the test runs
    with pytest.raises(SystemExit) as e:
        E.load_extractor(None, "cpu")
    msg = str(e.value)
    assert all(flag in msg for flag in ("--extractor", "--real-features", "--fake-features")) and msg.count(". ") == 0
    cfg = tmp_path / "tfds.yaml"
    cfg.write_text("name: t\nreal:\n  mode: tfds\n")
    with pytest.raises(SystemExit, match="TFDS"):
        E.main(["--config", str(cfg), "--fake", str(tmp_path)])
    with pytest.raises(ValueError, match="pkg.module:factory"):
        E.load_extractor("tests.eval_extractor", "cpu")
    assert callable(E.load_extractor("tests.eval_extractor:make", "cpu"))


def test_command_line_from_feature_files(tmp_path, monkeypatch, capsys):
    """--real-features / --fake-features: no extractor, no folders; the report's scores are full_evaluation's on the same features."""
    import json
    import numpy as np
    from gan_variant_research_amd import autograd as AG, evaluate as E
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: MifidEmuOps())
    r, f = N.features(20, 24, 12, seed=8)
    np.save(tmp_path / "real.npy", r)
    E.save_cached_stats("fake", tmp_path, r.mean(0), np.cov(r, rowvar=False), f, len(f))
    out = tmp_path / "o" / "report.json"
    assert E.main(["--real-features", str(tmp_path / "real.npy"), "--fake-features", str(tmp_path / "fake.npz"), "--out", str(out), "--device", "cpu",
                   "--cosine-eps", "0.5"]) == 0
    rep = json.load(open(out))
    fp = [f"{tmp_path / 'fake.npz'}#{i}" for i in range(len(f))]
    rp = [f"{tmp_path / 'real.npy'}#{i}" for i in range(len(r))]
    want = E.full_evaluation(r, f, fp, rp, 0.5, device="cpu", ops=MifidEmuOps())
    assert rep["scores"] == {"mifid": round(want["mifid"], 4), "fid": round(want["fid"], 4), "cosine_min_distance": want["cosine_min_distance"]}
    assert rep["memorization_analysis"]["worst_cases"] == want["worst_memorization_cases"]
    assert rep["run"]["num_fake"] == 24 and rep["run"]["num_real"] == 20 and (tmp_path / "o" / "report_worst_cases.csv").exists()


def test_c_entries_validate_before_they_launch():
    """The ABI contract of the evaluation entries, through ctypes as the decoders' tests do: every bad argument comes back as a non-zero
    code with a gan_last_error text that names it.  Validation fails before anything is launched or dereferenced, so no GPU is needed
    and the pointers are plain aligned numbers."""
    import ctypes as C
    from gan_variant_research_amd import _lib
    lib = _lib.load()
    P, Q = 1 << 20, (1 << 20) + 4                      # aligned; 4 off an 8-byte boundary
    F32, F64 = _lib.FEAT_F32, _lib.FEAT_F64
    err = lambda: lib.gan_last_error().decode()
    one = C.c_double(1.0)

    def gram(A=P, da=F32, lda=8, B=P, db=F32, ldb=8, trans=0, M=4, N=4, K=8, ca=None, cb=None, ra=None, rb=None, alpha=one, out=P, ldc=4):
        return lib.gan_gram_f64(A, da, lda, B, db, ldb, trans, M, N, K, ca, cb, ra, rb, alpha, out, ldc, None)

    for kw, text in ((dict(A=None), "null feature matrix"), (dict(B=None), "null feature matrix"), (dict(da=7), "dtype 7"),
                     (dict(lda=7), "row stride 7 below the 8 columns"), (dict(ldb=3, trans=1), "row stride 3 below the 4 columns"),
                     (dict(A=Q, da=F64), "misaligned feature matrix"), (dict(A=(1 << 20) + 2), "misaligned feature matrix"),
                     (dict(trans=2), "trans must be 0 or 1"), (dict(M=0), "extents must be positive"), (dict(K=-1), "extents must be positive"),
                     (dict(trans=1, ra=P), "row scales belong to trans = 0"), (dict(out=None), "null or misaligned output"),
                     (dict(out=Q), "null or misaligned output"), (dict(ldc=3), "output row stride 3 below the 4 columns"),
                     (dict(alpha=C.c_double(float("nan"))), "alpha is NaN"),
                     (dict(M=65535 * 64 + 1, lda=8), "beyond 65535 row tiles"),
                     (dict(N=2 ** 31 - 1), "are refused"), (dict(K=2 ** 31 - 1, lda=2 ** 31, ldb=2 ** 31), "are refused")):
        assert gram(**kw) != 0 and text in err(), (kw, err())

    def moments(X=P, dt=F32, n=4, D=8, ld=8, outs=(P,) * 6):
        return lib.gan_feat_moments(X, dt, n, D, ld, *outs, None)

    for kw, text in ((dict(X=None), "null feature matrix"), (dict(dt=-1), "dtype -1"), (dict(n=0), "extents must be positive"),
                     (dict(D=2 ** 31), "below 2^31"), (dict(ld=7), "row stride 7 below the 8 columns"), (dict(X=Q, dt=F64), "misaligned"),
                     (dict(outs=(P, P, None, P, P, P)), "null output"), (dict(outs=(P, P, P, P, P, None)), "null output")):
        assert moments(**kw) != 0 and text in err(), (kw, err())

    need = C.c_int64(0)
    assert lib.gan_cos_rowmin_bounds(70, 321, C.byref(need)) == 0 and need.value == 6 * 70 * 8 + 6 * 70 * 4
    assert lib.gan_cos_rowmin_bounds(3, 1, C.byref(need)) == 0 and need.value == 32 + 12          # the int32 part starts on a 16-byte boundary
    assert lib.gan_cos_rowmin_bounds(0, 5, C.byref(need)) != 0 and "extents must be positive" in err()
    assert lib.gan_cos_rowmin_bounds(5, 2 ** 31 - 1, C.byref(need)) != 0 and "are refused" in err()
    assert lib.gan_cos_rowmin_bounds(5, 5, None) != 0 and "null output" in err()

    def rowmin(A=P, lda=8, M=4, N=4, K=8, absolute=0, ws=P, ws_bytes=1 << 16, dmin=P, imin=P):
        return lib.gan_cos_rowmin(A, F32, lda, P, F32, 8, M, N, K, None, None, None, None, one, absolute, ws, ws_bytes, dmin, imin, None)

    for kw, text in ((dict(A=None), "null feature matrix"), (dict(lda=5), "row stride 5 below the 8 columns"), (dict(absolute=2), "absolute must be 0 or 1"),
                     (dict(dmin=None), "null output"), (dict(imin=None), "null output"), (dict(ws=None), "workspace"), (dict(ws=P + 8), "16-byte aligned"),
                     (dict(ws_bytes=47), "workspace of 47 bytes, gan_cos_rowmin_bounds asks 48"), (dict(M=65535 * 64 + 1), "beyond 65535 row tiles")):
        assert rowmin(**kw) != 0 and text in err(), (kw, err())

    assert lib.gan_input_pipeline_u8(None, None, 0, None, 16, 7, None, 0, None, None, None, None) != 0 and "filter" in err()
    assert lib.gan_input_pipeline_u8(None, None, 0, None, 16, 2, None, 0, None, None, None, None) != 0 and "null pointer or empty batch" in err()
