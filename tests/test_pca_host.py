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
