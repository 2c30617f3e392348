"""The checker of the PCA tests: correct.counts.using.PCA restated in numpy, line for line against the reference's
R/PCA_for_read_count.R:41-78 (R is not needed to run the tests, and nothing here comes from the library).  prcomp is
np.linalg.svd of the centred selected columns; round() is R's (IEC 60559 half-even) = np.rint."""
import numpy as np


def make_counts(E, S, seed, groups=True):
    """the parity tests' input: exon depths over two decades, 8 % near-empty exons, sample size factors, six batch groups"""
    rng = np.random.default_rng(seed)
    lam = rng.lognormal(np.log(90), 0.9, E)
    lam[rng.random(E) < 0.08] *= 0.01
    sf = rng.lognormal(0, 0.25, S)
    grp = rng.integers(0, 6, S)
    gn = rng.normal(0, 0.12, (E, 6))
    own = rng.normal(0, 0.05, (E, S))
    if not groups:
        return rng.poisson(lam[:, None] * sf[None, :]).astype(np.int32)
    return rng.poisson(lam[:, None] * sf[None, :] * np.exp(gn[:, grp] + own)).astype(np.int32)


def make_planted(E, S, k, seed, amp=0.6):
    """make_counts with the six batch groups replaced by k planted factors (a spectrum with k components above the noise, whatever k):
    rate x exp(F L + own), F ~ N(0, amp / sqrt(k)) (E x k), L ~ N(0, 1) (k x S).  Draw order: lam, the empty mask, sf, F, L, own, poisson."""
    rng = np.random.default_rng(seed)
    lam = rng.lognormal(np.log(90), 0.9, E)
    lam[rng.random(E) < 0.08] *= 0.01
    sf = rng.lognormal(0, 0.25, S)
    F = rng.normal(0, amp / np.sqrt(k), (E, k))
    L = rng.normal(0, 1, (k, S))
    own = rng.normal(0, 0.05, (E, S))
    return rng.poisson(lam[:, None] * sf[None, :] * np.exp(F @ L + own)).astype(np.int32)


def correct_counts_using_PCA(count_data, nPCs=3, mask_exons=None, sample_div=None, exon_mul=None, sample_mul=None, sd_min=2.0):
    C = np.asarray(count_data, dtype=np.float64)
    nexons, nsamples = C.shape                                      # :44-45
    my_rsums = C.sum(axis=1) / 1000.0                               # :50
    # :51  for (i in 1:nsamples) norm.count[,i] <- norm.count[,i] / max(1, my.rsums[i])   (per-exon vector, sample index)
    div = np.maximum(1.0, my_rsums[:nsamples]) if sample_div is None else np.asarray(sample_div, dtype=np.float64)
    norm = C / div[None, :]
    centers = norm.mean(axis=1)                                     # :55 colMeans of t(norm.count)
    sd = norm.std(axis=1, ddof=1)                                   # :56
    good_depth = sd > sd_min
    Z = norm - centers[:, None]                                     # :58
    sel = good_depth if mask_exons is None else (~np.asarray(mask_exons, dtype=bool) & good_depth)   # :63 / :65
    A = Z[sel].T                                                    # samples x selected exons
    A = A - A.mean(axis=0)                                          # prcomp's own centring (a no-op up to rounding)
    u, sv, _ = np.linalg.svd(A, full_matrices=False)
    PCA_mat = u[:, :nPCs] * sv[:nPCs]                               # :68 my.pca$x[, 1:nPCs]
    reg_mat = np.linalg.solve(PCA_mat.T @ PCA_mat, PCA_mat.T)       # :70
    coeff_mat = reg_mat @ Z.T                                       # :71
    resid = Z.T - PCA_mat @ coeff_mat                               # :72-74   samples x exons
    em = my_rsums if exon_mul is None else np.asarray(exon_mul, dtype=np.float64)
    sm = np.ones(nsamples) if sample_mul is None else np.asarray(sample_mul, dtype=np.float64)
    pre = (em[:, None] * sm[None, :]) * (resid.T + centers[:, None])    # :75 before pmax / round
    out = np.rint(np.maximum(0.0, pre))
    return {"out": out.astype(np.int64), "pre": pre, "selected": sel, "sd": sd, "centre": centers, "div": div, "rs": my_rsums,
            "theta": sv ** 2, "U": u[:, :nPCs]}


def preconditions(chk, nPCs, sd_min=2.0):
    """what has to hold of the CHECKER's own numbers for cell-for-cell equality to be a fair demand; returns the cells to leave out"""
    assert np.min(np.abs(chk["sd"] - sd_min)) > 1e-6, "an exon's sd within 1e-6 of sd_min"
    th = chk["theta"]
    assert th[nPCs - 1] / th[nPCs] >= 1.1, "theta_k / theta_k+1 = %g" % (th[nPCs - 1] / th[nPCs])
    p = np.maximum(chk["pre"], 0.0)
    near = np.abs(p - np.floor(p) - 0.5) < 1e-6
    assert near.sum() <= 10, "%d cells within 1e-6 of a half-integer" % near.sum()
    return near
