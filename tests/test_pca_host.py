"""correct_counts_using_PCA without a GPU: the argument errors raised in Python before the library is reached (the reference's own
checks, R/PCA_for_read_count.R:43, :60-61, with its messages), and no CPU fallback."""
import numpy as np
import pytest


def _counts(E=40, S=6):
    return np.random.default_rng(0).poisson(80.0, (E, S)).astype(np.int32)


def test_exported():
    import exomedepth_amd as ed
    for name in ("correct_counts_using_PCA", "pca_gram", "pca_last_info"):
        assert name in ed.__all__ and callable(getattr(ed, name))


def test_reference_input_checks_and_messages():
    import exomedepth_amd as ed
    C = _counts()
    with pytest.raises(ValueError, match="The input to the PCA correction must be a matrix"):
        ed.correct_counts_using_PCA(C[:, 0])
    with pytest.raises(ValueError, match="The input to the PCA correction must be a matrix"):
        ed.correct_counts_using_PCA([1, 2, 3])
    with pytest.raises(ValueError, match="The mask exons argument must be a logical vector"):
        ed.correct_counts_using_PCA(C, mask_exons=np.zeros(40, dtype=np.int32))
    with pytest.raises(ValueError, match="The length of the mask exons argument does not match the number of exons"):
        ed.correct_counts_using_PCA(C, mask_exons=np.zeros(39, dtype=bool))
    with pytest.raises(ValueError, match="must be a matrix"):
        ed.pca_gram(C.ravel())


def test_vector_shapes_are_checked_before_the_library():
    import exomedepth_amd as ed
    C = _counts()
    with pytest.raises(ValueError, match="sample_div must hold one value per sample"):
        ed.correct_counts_using_PCA(C, sample_div=np.ones(5))
    with pytest.raises(ValueError, match="exon_mul must hold one value per exon"):
        ed.correct_counts_using_PCA(C, exon_mul=np.ones(6))
    with pytest.raises(ValueError, match="sample_mul must hold one value per sample"):
        ed.correct_counts_using_PCA(C, sample_mul=np.ones(40))
    with pytest.raises(ValueError, match="out must have the shape"):
        ed.correct_counts_using_PCA(C, out=np.zeros((6, 40), dtype=np.int32))
    with pytest.raises(ValueError, match="out must be a device array"):
        ed.correct_counts_using_PCA(C, out=np.zeros((40, 6), dtype=np.int32))


def test_make_planted_is_deterministic():
    import pca_checker as pc
    a = pc.make_planted(120, 11, 4, 3)
    assert a.shape == (120, 11) and a.dtype == np.int32 and a.min() >= 0
    assert np.array_equal(a, pc.make_planted(120, 11, 4, 3))
    assert not np.array_equal(a, pc.make_planted(120, 11, 4, 4))
    assert not np.array_equal(a, pc.make_planted(120, 11, 4, 3, amp=0.5))
    # the first three draws are make_counts': with the factors switched off, what is left is the depths, the size factors and the exon's own noise
    flat = pc.make_planted(4000, 11, 4, 3, amp=0.0)
    assert abs(np.log(np.median(flat[flat.mean(axis=1) > 5])) - np.log(90)) < 0.2
    assert 0.04 < np.mean(flat.mean(axis=1) < 5) < 0.12


def test_geometry_inputs_meet_the_preconditions_the_gpu_tests_rely_on():
    """tests/test_gpu_pca_geometry.py's inputs, judged by the checker alone: most exons selected, no sd at the threshold, few cells at a
    half-integer, and cell-for-cell equality demanded exactly where theta_k / theta_k+1 >= 1.1 and theta_1 / theta_k < 100"""
    import pca_checker as pc
    from test_gpu_pca_geometry import MAX_SKIPPED, SHAPES, make_input, saturation_vectors
    assert len(set(s[:3] for s in SHAPES)) == len(SHAPES) == 14
    for E, S, k, gen, seed, cells in SHAPES:
        C = make_input(E, S, k, gen, seed)
        assert C.shape == (E, S) and k < S <= E
        chk = pc.correct_counts_using_PCA(C, k)
        th = chk["theta"]
        assert chk["selected"].mean() >= 0.85, (E, S, k)
        assert k < chk["selected"].sum()
        assert np.min(np.abs(chk["sd"] - 2.0)) > 1e-6, (E, S, k)
        p = np.maximum(chk["pre"], 0.0)
        assert (np.abs(p - np.floor(p) - 0.5) < 1e-6).sum() <= MAX_SKIPPED, (E, S, k)
        assert chk["pre"].max() < 2147483647.0
        assert th[k - 1] > 0.0
        fair = bool(th[k - 1] >= 1.1 * th[k] and th[0] < 100.0 * th[k - 1])
        assert fair == cells, (E, S, k, th[k - 1] / th[k], th[0] / th[k - 1])
        if cells:
            pc.preconditions(chk, k)
    C = pc.make_counts(300, 24, 5)
    em, sm, rows = saturation_vectors(pc.correct_counts_using_PCA(C, 2))
    assert len(set(rows.values())) == 5 and (sm == 0).sum() == 2
    assert em[rows["zero"]] == 0 and em[rows["big"]] == 1e12 and em[rows["inf"]] == np.inf and em[rows["inf_mixed"]] == np.inf and em[rows["neg"]] == -1


def test_no_cpu_fallback():
    import __graft_entry__ as g
    g.build()
    import exomedepth_amd as ed
    from exomedepth_amd import EdError, _lib
    if _lib.lib().ed_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(EdError, match="no usable HIP device"):
        ed.correct_counts_using_PCA(_counts())
    with pytest.raises(EdError, match="no usable HIP device"):
        ed.pca_gram(_counts())
