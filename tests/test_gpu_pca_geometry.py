"""correct_counts_using_PCA, the whole call, at the sizes where its kernels change path (csrc/edpca.inc): the block width b = min(S, max(2k, k + 8))
at 54 / 56 (dynamic LDS of k_pca_jacobi / k_pca_chol past 48 KiB), 90 / 92 (the rotations and R^-1 leave LDS for global memory), 128 (one b x b
matrix is 128 KiB); S k doubles at and past the 64 KiB of k_pca_residual's LDS copy of U (S = 1024 / 1025, k = 8; S = 129, k = 64); b clamped to S
(S = 9, 6, 2, 128; k = S - 1); S > 128 (more than one Gram tile); E = 1025 (k_pca_compact's clamped ranges).  tests/test_pca_host.py checks the
inputs' preconditions without a GPU.

Per shape, against numpy on the host (never the library): the device's eigenpairs against pca_gram's G (residual, orthonormality, eigenvalues
against eigvalsh, the subspace against numpy's within the Davis-Kahan bound), every output cell against the rounding rule applied to the value before
rounding recomputed from the device's own U, and -- where theta_k / theta_k+1 >= 1.1 and theta_1 / theta_k < 100 -- every cell against the checker.

Per-shape figures on the MI355X (iterations, residual, skipped cells, max |device - numpy|): NOT MEASURED.  These tests have not run on a
device yet; test_whole_call prints the figures ("PCA geometry ..." lines, pytest -s) and they belong here and in DESIGN.md 4.14 once they have.
Whether k_pca_jacobi / k_pca_chol are launched with 64 - 128 KiB of dynamic LDS, and k_pca_residual with exactly 64 KiB, is what the
b >= 65 and S k = 8192 cases find out."""
import math

import numpy as np
import pytest

import pca_checker as pc
from test_gpu_pca import _assert_equal_cells, _device_pre

pytestmark = pytest.mark.gpu

# (E, S, k, generator, seed, cell for cell against the checker)
SHAPES = [
    (50, 2, 1, "counts", 8, True),
    (400, 9, 1, "planted", 1010, True),
    (300, 6, 5, "planted", 1011, True),
    (600, 65, 27, "planted", 1092, False),
    (600, 65, 28, "planted", 1093, False),
    (700, 100, 45, "planted", 1145, False),
    (700, 100, 46, "planted", 1146, False),
    (900, 128, 64, "planted", 1192, False),
    (900, 129, 64, "planted", 1193, False),
    (1200, 257, 9, "planted", 1266, True),
    (1025, 257, 9, "planted", 1266, True),
    (1100, 1024, 8, "planted", 2032, True),
    (1100, 1025, 8, "planted", 2033, True),
    (1100, 1025, 9, "planted", 2034, True),
]
MAX_SKIPPED = 10
_cache = {}


def make_input(E, S, k, gen, seed):
    return pc.make_planted(E, S, k, seed) if gen == "planted" else pc.make_counts(E, S, seed)


def _case(E, S, k, gen, seed):
    """(counts, checker result), computed once and shared (read-only)"""
    key = (E, S, k, gen, seed)
    if key not in _cache:
        C = make_input(E, S, k, gen, seed)
        C.setflags(write=False)
        _cache[key] = (C, pc.correct_counts_using_PCA(C, k))
    return _cache[key]


def _rounding_budget(C, chk, U, k, exon_mul=None, sample_mul=None):
    """64 x the rounding budget of k_pca_residual's summation order for the value before rounding: (ceil(S / 64) + k + 8) 2^-53
    m (|z| + sum_j |U_sj| sum_s' |U_s'j| |z_s'| + |centre|), m = |exon_mul sample_mul|"""
    S = C.shape[1]
    Z = np.abs(np.asarray(C, dtype=np.float64) / chk["div"][None, :] - chk["centre"][:, None])
    A = np.abs(U)
    em = chk["rs"] if exon_mul is None else exon_mul
    sm = np.ones(S) if sample_mul is None else sample_mul
    m = np.abs(em[:, None] * sm[None, :])
    return 64.0 * (math.ceil(S / 64) + k + 8) * 2.0 ** -53 * m * (Z + (Z @ A) @ A.T + np.abs(chk["centre"])[:, None])


def _near_half(pre, err):
    p = np.maximum(pre, 0.0)
    return np.abs(p - np.floor(p) - 0.5) <= err


@pytest.mark.parametrize("E,S,k,gen,seed,cells", SHAPES, ids=["%dx%d-k%d" % s[:3] for s in SHAPES])
def test_whole_call(edlib, E, S, k, gen, seed, cells):
    ed = edlib
    C, chk = _case(E, S, k, gen, seed)
    b = min(S, max(2 * k, k + 8))
    got = ed.correct_counts_using_PCA(C, k).to_host()
    info = ed.pca_last_info()
    g = ed.pca_gram(C)
    assert got.shape == (E, S)
    assert np.array_equal(g["selected"], chk["selected"]) and info["n_selected"] == g["n_selected"] == int(chk["selected"].sum())
    assert info["block"] == b and info["nPCs"] == k and info["converged"]
    assert 1 <= info["iterations"] <= 500 and info["residual"] <= 1e-12

    # ---- stage 3: the eigenpairs against G itself; none of this depends on theta_k / theta_k+1
    G, U, th = g["G"], info["U"], info["theta"]
    assert U.shape == (S, k) and th.shape == (k + 1,) and np.all(np.isfinite(U)) and np.all(np.isfinite(th))
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1], V[:, ::-1]
    Gl, Ul = G.astype(np.longdouble), U.astype(np.longdouble)
    resid = np.sqrt(((Gl @ Ul - Ul * th[None, :k].astype(np.longdouble)) ** 2).sum(axis=0)).astype(np.float64)
    orth = np.max(np.abs(U.T @ U - np.eye(k)))
    dth = np.max(np.abs(th[:k] - lam[:k]))
    assert np.all(resid <= 1e-12 * th[0]), "residual %.3e of theta_1" % (resid.max() / th[0])
    assert orth <= 1e-12
    assert dth <= 2e-12 * lam[0]
    assert np.all(np.diff(th[:k]) <= 0)
    angle = bound = float("nan")
    if th[k - 1] > th[k]:
        angle = np.linalg.norm(U @ U.T - V[:, :k] @ V[:, :k].T, 2)
        bound = 2.0 * math.sqrt(k) * 1e-12 * lam[0] / (lam[k - 1] - lam[k])
        assert angle <= bound
    if th[k] > 0.0:
        assert info["gap"] == th[k - 1] / th[k]
    if b == S:
        # the basis spans the whole space: theta[k] is an eigenvalue of G and not a Ritz value of a subspace
        assert info["gap"] > 0.0 and not math.isnan(info["gap"])
        if k < S - 1:
            assert math.isfinite(info["gap"]) and abs(th[k] - lam[k]) <= 2e-12 * lam[0]
        else:
            # theta_S of a centred Gram matrix is zero in exact arithmetic.  What is computed is rounding of either sign (a value <= 0 is
            # reported as an infinite ratio): at most |dG|_2 <= (n + 8) 2^-53 trace(H), the bound of test_gram_accuracy_and_geometry, plus
            # the 2e-12 lambda_1 allowed to an eigenvalue above
            N = np.asarray(C, dtype=np.float64)[chk["selected"]] / chk["div"][None, :]
            trace_h = ((np.abs(N) + np.abs(chk["centre"][chk["selected"]])[:, None]) ** 2).sum()
            assert abs(th[k]) <= (g["n_selected"] + 8) * 2.0 ** -53 * trace_h + 2e-12 * lam[0]
            assert info["gap"] >= th[k - 1] / ((g["n_selected"] + 8) * 2.0 ** -53 * trace_h + 2e-12 * lam[0])

    # ---- stage 4: the rounding rule on the value before rounding recomputed from the device's own U
    dpre = _device_pre(C, chk, info)
    err = _rounding_budget(C, chk, U, k)
    skip = _near_half(dpre, err)
    want = np.rint(np.maximum(0.0, dpre)).astype(np.int64)
    assert dpre.max() < 2147483647.0
    bad = (got != want) & ~skip
    print("PCA geometry E=%d S=%d k=%d b=%d: iterations %d, residual %.3e (recomputed %.3e), |U'U - I| %.1e, |theta - lambda| / lambda_1 %.1e, "
          "angle %.3e (bound %.3e), gap %.4g, skipped cells %d, max |device - numpy| = %d, max |device pre-round - checker| = %.3e"
          % (E, S, k, b, info["iterations"], info["residual"], resid.max() / th[0], orth, dth / lam[0], angle, bound, info["gap"], skip.sum(),
             np.max(np.abs(got - want)), np.max(np.abs(dpre - chk["pre"]))))
    assert skip.sum() <= MAX_SKIPPED, "%d cells within the rounding budget of a half-integer" % skip.sum()
    assert not bad.any(), "%d cells differ from the rule, first at %s: %d vs %d (before rounding %r)" % (
        bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0], dpre[bad][0])

    # ---- cell for cell against the checker, where its own spectrum makes that a fair demand
    if cells:
        th_c = chk["theta"]
        assert th_c[0] / th_c[k - 1] < 100.0
        _assert_equal_cells(got, chk, pc.preconditions(chk, k))


def saturation_vectors(chk):
    """exon_mul (the default rs with six entries replaced) and sample_mul (ones with two zeros) of the saturation test, and the rows replaced.
    The rows are picked from the checker's value before scaling, v = residual + centre: 1e12 and +inf on rows with every v > 1 (every cell
    overflows), a second +inf and the -1 on rows (near-empty exons) where v is below -0.6 in one sample -- -v then rounds to 1 -- and positive in
    another, no |v| below 1e-3 (the device's v is within 1e-6 of the checker's, test_gpu_pca.py: the signs are the same)."""
    v = chk["pre"] / chk["rs"][:, None]
    E, S = v.shape
    high = np.flatnonzero(v.min(axis=1) > 1.0)
    live = np.ones(S, dtype=bool)
    live[[3, S - 1]] = False                 # sample_mul's zeros
    mixed = np.flatnonzero((v[:, live].min(axis=1) < -0.6) & (v[:, live].max(axis=1) > 1e-3) & (np.abs(v).min(axis=1) > 1e-3))
    assert high.size >= 3 and mixed.size >= 2, "the generator gave too few rows of the kinds the test needs"
    rows = {"zero": int(high[0]), "big": int(high[1]), "inf": int(high[2]), "inf_mixed": int(mixed[0]), "neg": int(mixed[1])}
    em = chk["rs"].copy()
    em[rows["zero"]] = 0.0
    em[rows["big"]] = 1e12
    em[rows["inf"]] = em[rows["inf_mixed"]] = np.inf
    em[rows["neg"]] = -1.0
    sm = live.astype(np.float64)
    return em, sm, rows


def test_saturation_and_multipliers(edlib):
    """stage 4's rule out = rint(min(2147483647, max(0, v))), a NaN v (inf x 0) giving 0, with v = exon_mul sample_mul (residual + centre)"""
    ed = edlib
    E, S, k, seed = 300, 24, 2, 5
    C, chk = _case(E, S, k, "counts", seed)
    em, sm, rows = saturation_vectors(chk)
    plain = ed.correct_counts_using_PCA(C, k).to_host()
    got = ed.correct_counts_using_PCA(C, k, exon_mul=em, sample_mul=sm).to_host()
    info = ed.pca_last_info()
    with np.errstate(invalid="ignore", over="ignore"):
        dpre = _device_pre(C, chk, info, exon_mul=em, sample_mul=sm)
        err = _rounding_budget(C, chk, info["U"], k, exon_mul=em, sample_mul=sm)
        want = np.rint(np.minimum(2147483647.0, np.maximum(0.0, dpre)))
        want[np.isnan(dpre)] = 0.0
        skip = np.isfinite(dpre) & (dpre < 2147483647.0) & _near_half(dpre, err)
    want = want.astype(np.int64)
    live = sm != 0.0
    print("PCA saturation: %d NaN, %d clamped at 2^31 - 1, %d negative, skipped cells %d"
          % (np.isnan(dpre).sum(), (dpre >= 2147483647.0).sum(), (dpre < 0).sum(), skip.sum()))
    assert skip.sum() <= MAX_SKIPPED
    assert np.array_equal(got[~skip], want[~skip])
    # the named cases, each stated on its own
    assert np.isnan(dpre[rows["inf"], ~live]).all() and np.isnan(dpre[rows["inf_mixed"], ~live]).all()
    assert (got[:, ~live] == 0).all(), "sample_mul = 0 (and inf x 0 = NaN) must give 0"
    assert (got[rows["zero"]] == 0).all()
    assert (got[rows["big"], live] == 2147483647).all() and (got[rows["inf"], live] == 2147483647).all()
    v = chk["pre"] / chk["rs"][:, None]
    assert np.array_equal(got[rows["inf_mixed"], live], np.where(v[rows["inf_mixed"], live] > 0, 2147483647, 0))
    vn, gn = v[rows["neg"], live], got[rows["neg"], live]
    assert (gn[vn > 0] == 0).all() and (gn[vn < -0.6] >= 1).all() and (vn > 0).any() and (vn < -0.6).any()
    assert got.min() == 0 and got.max() == 2147483647
    # rows and columns whose multipliers are the defaults: the plain call's bits
    untouched = np.ones(E, dtype=bool)
    untouched[list(rows.values())] = False
    assert np.array_equal(got[np.ix_(untouched, live)], plain[np.ix_(untouched, live)])
