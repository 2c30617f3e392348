"""correct_counts_using_PCA on the device against the numpy restatement of R/PCA_for_read_count.R (tests/pca_checker.py).

Cell-for-cell equality is demanded wherever the checker's own numbers make it a fair demand (pca_checker.preconditions): no exon's sd within 1e-6
of sd_min, theta_k / theta_k+1 >= 1.1, and at most 10 cells whose value before rounding lies within 1e-6 of a half-integer (those cells are left
out).  1e-6: a subspace converged to 1e-12 theta_1 with such gaps moves a value before rounding by about 1e-8.  Measured (MI355X): the largest
|device value before rounding - checker's| is 5.8e-7 / 1.0e-6 / 8.6e-7 / 3.9e-7 on the four parity shapes after 12 / 9 / 9 / 10 iterations (theta_1 is
decades above theta_k); test_parity prints it.  Defaults on (6000, 48, 5): 9 iterations, residual 1.2e-13."""
import numpy as np
import pytest

import pca_checker as pc

pytestmark = pytest.mark.gpu

PARITY = [(3000, 24, 3, 1), (4099, 37, 3, 2), (6000, 48, 5, 3), (2500, 70, 2, 4)]
_cache = {}


def _case(E, S, k, seed):
    """(counts, checker result), computed once and shared (read-only) by the tests that need it"""
    key = (E, S, k, seed)
    if key not in _cache:
        C = pc.make_counts(E, S, seed)
        C.setflags(write=False)
        _cache[key] = (C, pc.correct_counts_using_PCA(C, k))
    return _cache[key]


def _assert_equal_cells(got, chk, near):
    bad = (got != chk["out"]) & ~near
    assert not bad.any(), "%d cells differ, first at %s: %s vs %s (before rounding %r)" % (
        bad.sum(), np.argwhere(bad)[0], got[bad][0], chk["out"][bad][0], chk["pre"][bad][0])


def _device_pre(C, chk_like, info, exon_mul=None, sample_mul=None):
    """the device's value before rounding, recomputed in numpy from the device's own eigenvectors"""
    U = info["U"]
    Z = np.asarray(C, dtype=np.float64) / chk_like["div"][None, :] - chk_like["centre"][:, None]
    R = Z - (Z @ U) @ U.T
    em = chk_like["rs"] if exon_mul is None else exon_mul
    sm = np.ones(C.shape[1]) if sample_mul is None else sample_mul
    return (em[:, None] * sm[None, :]) * (R + chk_like["centre"][:, None])


@pytest.mark.parametrize("E,S,k,seed", PARITY)
def test_parity(edlib, E, S, k, seed):
    ed = edlib
    C, chk = _case(E, S, k, seed)
    near = pc.preconditions(chk, k)
    res = ed.correct_counts_using_PCA(C, k)
    assert res.shape == (E, S) and res.host_dtype == np.int32
    got = res.to_host()
    info = ed.pca_last_info()
    g = ed.pca_gram(C)
    assert np.array_equal(g["selected"], chk["selected"])
    assert info["n_selected"] == int(chk["selected"].sum()) == g["n_selected"]
    assert info["block"] == min(S, max(2 * k, k + 8)) and info["nPCs"] == k
    assert info["residual"] <= 1e-12 and 1 <= info["iterations"] <= 500
    dpre = _device_pre(C, chk, info)
    print("PCA parity E=%d S=%d k=%d: iterations %d, residual %.3e, gap %.4f, max |device pre-round - checker| = %.3e, clamped %.2f %%, good %.1f %%"
          % (E, S, k, info["iterations"], info["residual"], info["gap"], np.max(np.abs(dpre - chk["pre"])), 100.0 * np.mean(chk["pre"] < 0),
             100.0 * np.mean(chk["selected"])))
    assert np.allclose(info["theta"][:k], chk["theta"][:k], rtol=1e-9, atol=0)
    _assert_equal_cells(got, chk, near)


def test_mask(edlib):
    ed = edlib
    E, S, k, seed = 4099, 37, 3, 2
    C, plain = _case(E, S, k, seed)
    mask = np.random.default_rng(77).random(E) < 0.2
    chk = pc.correct_counts_using_PCA(C, k, mask_exons=mask)
    near = pc.preconditions(chk, k)
    got = ed.correct_counts_using_PCA(C, k, mask_exons=mask).to_host()
    assert ed.pca_last_info()["n_selected"] == int(chk["selected"].sum())
    assert np.array_equal(ed.pca_gram(C, mask_exons=mask)["selected"], chk["selected"])
    _assert_equal_cells(got, chk, near)
    unmasked = ed.correct_counts_using_PCA(C, k).to_host()
    assert not np.array_equal(got, unmasked)
    assert (got[mask] != C[mask]).any(), "masked exons are still corrected"


GRAM = [(2, 1), (15, 3), (16, 4), (17, 5), (33, 15), (64, 16), (65, 17), (129, 223), (33, 224), (129, 225)]


@pytest.mark.parametrize("S,n", GRAM)
def test_gram_accuracy_and_geometry(edlib, S, n):
    """G against the same sum in long double: |dG_ab| <= (n + 8) 2^-53 sqrt(H_aa H_bb), H the Gram matrix of |c| / div + |centre| over the
    selected rows (the inner-product bound + the rounding of forming z).  S around the MFMA block (16), the wave's tile (64) and the workgroup's
    (128); n = 1, 3, 4, 5 around the k-step of 4, 15 / 16 / 17 around the 16 rows staged at a time = one slice's worth while n <= 224,
    223 / 224 / 225 around every slice holding exactly one."""
    ed = edlib
    E = 700
    C = pc.make_counts(E, S, 100 + S)
    base = pc.correct_counts_using_PCA(C, 1)
    good = np.flatnonzero(base["selected"])
    assert good.size >= n, "the generator gave too few exons above sd_min"
    mask = np.ones(E, dtype=bool)
    mask[good[:n]] = False                      # exactly the first n good exons stay selected
    g = ed.pca_gram(C, mask_exons=mask)
    assert g["n_selected"] == n and np.array_equal(np.flatnonzero(g["selected"]), good[:n])
    assert np.array_equal(g["div"], base["div"])
    G = g["G"]
    assert np.array_equal(G, G.T)
    assert np.array_equal(G.view(np.int64), ed.pca_gram(C, mask_exons=mask)["G"].view(np.int64))
    Cl = C[good[:n]].astype(np.longdouble)
    Nl = Cl / base["div"].astype(np.longdouble)[None, :]
    cl = Nl.mean(axis=1)
    Zl = Nl - cl[:, None]
    Gl = Zl.T @ Zl
    Hm = np.abs(Nl) + np.abs(cl)[:, None]
    H = Hm.T @ Hm
    bound = (n + 8) * 2.0 ** -53 * np.sqrt(np.outer(np.diag(H), np.diag(H)))
    err = np.abs(G.astype(np.longdouble) - Gl)
    print("Gram S=%d n=%d: max err / bound = %.3f" % (S, n, float(np.max(err / bound))))
    assert np.all(err <= bound)
    # centre: S divisions (1 rounding each), a sum of at most ceil(S / 64) + 6 additions deep, one division: within 16 roundings of the mean of |N|
    assert np.all(np.abs(g["centre"][good[:n]] - cl.astype(np.float64)) <= 16 * 2.0 ** -53 * np.abs(Nl).mean(axis=1).astype(np.float64))


def test_explicit_vectors_equal_to_the_defaults_give_the_same_bits(edlib):
    ed = edlib
    C, chk = _case(*PARITY[0])
    a = ed.correct_counts_using_PCA(C, 3).to_host()
    b = ed.correct_counts_using_PCA(C, 3, sample_div=chk["div"], exon_mul=chk["rs"], sample_mul=np.ones(C.shape[1])).to_host()
    assert np.array_equal(a, b)


def test_per_sample_depth_vectors(edlib):
    ed = edlib
    E, S, k, seed = 4099, 37, 3, 2
    C, _ = _case(E, S, k, seed)
    dv = np.maximum(1.0, C.sum(axis=0) / 1000.0)
    ones = np.ones(E)
    sd = pc.correct_counts_using_PCA(C, k, sample_div=dv, exon_mul=ones, sample_mul=dv, sd_min=0.0)["sd"]
    srt = np.sort(sd)
    i = int(0.1 * E)
    while srt[i + 1] - srt[i] < 1e-5:          # a threshold clear (1e-6, the precondition) of every exon's sd, about 90 % of the exons above it
        i += 1
    sd_min = 0.5 * (srt[i] + srt[i + 1])
    chk = pc.correct_counts_using_PCA(C, k, sample_div=dv, exon_mul=ones, sample_mul=dv, sd_min=sd_min)
    assert 0.85 < chk["selected"].mean() < 0.95
    near = pc.preconditions(chk, k, sd_min)
    got = ed.correct_counts_using_PCA(C, k, sample_div=dv, exon_mul=ones, sample_mul=dv, sd_min=sd_min).to_host()
    assert ed.pca_last_info()["n_selected"] == int(chk["selected"].sum())
    _assert_equal_cells(got, chk, near)


def test_one_iteration_is_an_error_not_an_answer(edlib):
    ed = edlib
    C, _ = _case(*PARITY[2])
    with pytest.raises(ed.EdError, match=r"did not converge: 1 iterations, residual [0-9.e+-]+ of theta_1 .*theta_k / theta_k\+1"):
        ed.correct_counts_using_PCA(C, 5, max_iter=1)
    ed.correct_counts_using_PCA(C, 5)             # the device is fine afterwards, and the defaults converge
    info = ed.pca_last_info()
    print("PCA defaults on (6000, 48, 5): %d iterations, residual %.3e" % (info["iterations"], info["residual"]))
    assert info["residual"] <= 1e-12


def test_no_structure_converges_or_raises(edlib):
    """pure Poisson, no group structure: theta_k / theta_k+1 is close to 1.  Either outcome passes -- an error, or eigenvectors that meet
    |G U - U Theta| <= tol theta_1 recomputed here from pca_gram's G."""
    ed = edlib
    C = pc.make_counts(2500, 70, 9, groups=False)
    try:
        ed.correct_counts_using_PCA(C, 2)
    except ed.EdError as e:
        assert "did not converge" in str(e)
        print("no-structure cohort: raised: %s" % e)
        return
    info = ed.pca_last_info()
    G = ed.pca_gram(C)["G"]
    U, th = info["U"], info["theta"]
    r = np.linalg.norm(G @ U - U * th[None, :2], axis=0)
    print("no-structure cohort: converged in %d iterations, residual %.3e (numpy %.3e), gap %.4f"
          % (info["iterations"], info["residual"], r.max() / th[0], info["gap"]))
    assert r.max() <= 1e-12 * th[0]
    assert np.allclose(U.T @ U, np.eye(2), atol=1e-12)


def test_determinism_and_plumbing(edlib):
    import torch
    ed = edlib
    E, S, k, seed = PARITY[0]
    C, chk = _case(E, S, k, seed)
    res = ed.correct_counts_using_PCA(C, k)
    a = res.to_host()
    assert np.array_equal(a, ed.correct_counts_using_PCA(C, k).to_host())
    st = torch.cuda.Stream()
    ct = torch.from_numpy(np.array(C)).cuda()
    out = torch.zeros_like(ct)
    torch.cuda.synchronize()
    ret = ed.correct_counts_using_PCA(ct, k, out=out, stream=st.cuda_stream)
    assert ret is out
    assert np.array_equal(out.cpu().numpy(), a)
    sets = ed.cohort_select_reference_sets(res, want_reference=True)
    assert sets["n_chosen"].shape == (S,) and (sets["n_chosen"] >= 1).all()
    assert sets["reference"].to_host().shape == (E, S)


def test_invalid_arguments(edlib):
    ed = edlib
    C, _ = _case(*PARITY[0])
    E, S = C.shape
    cases = [
        (dict(count_data=C, nPCs=0), "nPCs = 0, at least 1"),
        (dict(count_data=pc.make_counts(300, 70, 5), nPCs=65), "nPCs = 65, at most 64"),
        (dict(count_data=C, nPCs=S), "nPCs = 24 must be below the number of samples"),
        (dict(count_data=C[:5, :8], nPCs=1), "needs n_samples <= n_exons"),
        (dict(count_data=np.zeros((1, 32769), dtype=np.int32), nPCs=1), "at most 32768 per call"),
        (dict(count_data=np.full((50, 6), 7, dtype=np.int32), nPCs=1), "no exon has a standard deviation above sd_min = 2"),
        (dict(count_data=C, nPCs=1, sample_div=np.r_[np.ones(S - 1), 0.0]), r"sample_div\[23\] = 0: the divisors must be finite and positive"),
        (dict(count_data=C, nPCs=1, sample_div=np.r_[np.inf, np.ones(S - 1)]), r"sample_div\[0\] = inf: the divisors must be finite and positive"),
    ]
    for kw, msg in cases:
        with pytest.raises(ed.EdError, match=msg) as ei:
            ed.correct_counts_using_PCA(**kw)
        assert "status -1" in str(ei.value), str(ei.value)
    # nPCs >= the number of selected exons: all but two good exons masked
    good = np.flatnonzero(pc.correct_counts_using_PCA(C, 1)["selected"])
    mask = np.ones(E, dtype=bool)
    mask[good[:2]] = False
    with pytest.raises(ed.EdError, match=r"nPCs = 3 must be below the number of selected exons \(2\)"):
        ed.correct_counts_using_PCA(C, 3, mask_exons=mask)
    with pytest.raises(ed.EdError, match="no exon has a standard deviation above sd_min = 2 outside the mask"):
        ed.correct_counts_using_PCA(C, 1, mask_exons=np.ones(E, dtype=bool))
