"""Inputs of tests/test_gpu_emit_geometry.py: the depth-binned (`phi.bins > 1`) and covariate models at the edges of their kernels.
numpy only; every case is a function of its arguments and a seed.  tests/test_emit_geometry_host.py verifies, on the CPU and with the
checker alone, that each case is what the GPU tests take it for.

Emission cases carry hand-set parameters (no fit stands between the inputs and the likelihoods) and reference counts planted on
every branch of bins_phi_linear and on both sides of the table of constants (kBinsRtab = 8192 reference counts; csrc/edbins.inc)."""
import numpy as np

RTAB = 8192                 # kBinsRtab (csrc/edcore.hip): reference counts covered by the table of constants
TILE_ROWS = 4               # exon rows of a workgroup tile (kEmitBlock / 64)
TILES_PER_WG = 32           # tiles a workgroup of k_emit_bins walks behind k_emit_bins_tab
FAR = 200000                # "one count near 200 000"

# (E, S, B, chromosome sizes): every B in 2..8 once; (4, 64) has an empty chromosome
BINS_SHAPES = ((1, 1, 2, (1,)), (3, 65, 3, (2, 1)), (4, 64, 4, (1, 0, 3)), (5, 63, 5, (5,)), (130, 130, 6, (50, 80)),
               (258, 2, 7, (100, 30, 128)), (1027, 65, 8, (500, 527)))
FOLD_SHAPE = (262145, 2, 3, (65536, 65537, 3, 131069))      # eblk = 65537: gridDim.z = 2 in both emission launches
# (E, S, K, chromosome sizes)
COV_SHAPES = ((3, 65, 1, (2, 1)), (5, 63, 0, (5,)), (130, 130, 3, (50, 80)), (1027, 2, 2, (500, 527)))


def design(sizes, seed):
    """(chrom_off, start, end): exons ordered by position inside each chromosome, every exon with its own gap to the next"""
    sizes = [int(n) for n in sizes]
    E = sum(sizes)
    rng = np.random.default_rng([seed, 11])
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    gaps = rng.integers(100, 9000, E)
    start = np.zeros(E, dtype=np.int64)
    for c in range(len(sizes)):
        lo, hi = chrom_off[c], chrom_off[c + 1]
        start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
    end = start + rng.integers(50, 400, E)
    return chrom_off, start.astype(np.int32), end.astype(np.int32)


def midpoints(edges):
    B = edges.shape[0] - 1
    return (edges[:B] + edges[1:B + 1]) / 2


def bins_params(S, B, seed, ood_sample=None):
    """hand-set (phi_bins (B, S), edges (B + 1, S), expected (S)).  edges[k] = k * by for k < B.  Three samples in four have an even
    integer `by` (integer mid-points) and a last edge that makes the LAST mid-point a half-integer; every fourth sample has by = even + 0.5
    (no integer mid-point, fractional edges)."""
    rng = np.random.default_rng([seed, 12])
    s = np.arange(S)
    by = 2.0 * (8 + (s * 7) % 23) + np.where(s % 4 == 3, 0.5, 0.0)
    edges = np.arange(B + 1, dtype=np.float64)[:, None] * by[None, :]
    edges[B] = edges[B - 1] + 2 * (5 + s % 9) + 1          # odd distance: (edges[B-1] + edges[B]) / 2 is no integer
    phi_bins = rng.uniform(0.002, 0.05, (B, S))
    expected = rng.uniform(0.08, 0.55, S)
    if ood_sample is not None:
        phi_bins[min(1, B - 1), ood_sample] = 1.5            # out of the domain: phi.linear crosses 1 between two mid-points
    return phi_bins, edges, expected


def plant_values(edges_s):
    """reference counts of one sample that land on every branch of bins_phi_linear and on both sides of the table:
    list of (name, value)"""
    mid = midpoints(edges_s)
    out = [("zero", 0)]
    for g, m in enumerate(mid):
        if m == np.floor(m):
            out += [("mid%d" % g, int(m)), ("mid%d-1" % g, int(m) - 1), ("mid%d+1" % g, int(m) + 1)]
        else:
            out += [("mid%d.floor" % g, int(np.floor(m))), ("mid%d.ceil" % g, int(np.ceil(m)))]
    for k, e in enumerate(edges_s):
        out += [("edge%d" % k, int(np.floor(e)))] + ([("edge%d.ceil" % k, int(np.ceil(e)))] if e != np.floor(e) else [])
    out += [("below", max(int(np.floor(mid[0])) - 3, 0)), ("above", int(np.ceil(mid[-1])) + 7)]
    out += [("rtab-1", RTAB - 1), ("rtab", RTAB), ("rtab+1", RTAB + 1), ("far", FAR)]
    return out


BIG_NAMES = ("rtab", "rtab+1", "far")


def _counts(E, S, edges, expected, rng):
    """seeded background: reference counts over (and a little beyond) the levels, test counts binomial around `expected`, and a
    block of halved / 1.5-fold test counts per sample where there is room for one"""
    top = edges[-1][None, :] * 1.3
    ref = np.floor(rng.uniform(0.0, 1.0, (E, S)) * top).astype(np.int64)
    odds = expected / (1.0 - expected)
    test = rng.poisson(np.maximum(ref * odds[None, :], 0.5)).astype(np.int64)
    if E >= 12:
        for s in range(S):
            for rep in range(max(1, E // 120)):
                a = int(rng.integers(0, E - 8)); n = int(rng.integers(4, 9))
                f = 0.5 if (s + rep) % 2 == 0 else 1.5
                test[a:a + n, s] = np.floor(test[a:a + n, s] * f)
                ref[a:a + n, s] = np.maximum(ref[a:a + n, s], 40)
    return test, ref


def _test_for(ref_value, ex, rng):
    return int(rng.poisson(max(ref_value * ex / (1.0 - ex), 0.5)))


def big_rows(E):
    """rows reserved for the planted counts >= RTAB at E = 130 and 258 (tile = row // 4; workgroup of k_emit_bins = tile // 32):
    two tiles of workgroup 0 that every sample fills, the last exon (partial tile, partial workgroup), and rows where single samples go"""
    r = {"all_a": 4 * 2 + 1, "all_b": 4 * 9 + 2, "all_far": E - 1, "first_lane": 4 * 5 + 0, "last_lane": 4 * 7 + 3, "last_row": 4 * 12 + 3,
         "walk_end": 4 * 31 + 2}       # tile 31: the last of the 32 a workgroup walks
    if E > 4 * 40 + 2:
        r["second_wg"] = 4 * 40 + 2
    return r


def bins_emit_case(E, S, B, sizes, seed, ood_sample=None, placed=None):
    """One emission case of the depth-binned model.  `placed` (default: E in (130, 258)): the counts >= RTAB go to the rows of big_rows()
    so that whole tiles have none, some have exactly one and the partial workgroup has some; otherwise every sample's plants go to
    random distinct rows (or, where a sample has fewer rows than plants, the plants are dealt round the samples)."""
    assert sum(sizes) == E
    if placed is None:
        placed = E in (130, 258)
    rng = np.random.default_rng([seed, 13])
    chrom_off, start, end = design(sizes, seed)
    phi_bins, edges, expected = bins_params(S, B, seed, ood_sample)
    test, ref = _counts(E, S, edges, expected, rng)
    planted = [dict() for _ in range(S)]          # name -> row
    rows_big = big_rows(E) if placed else {}
    reserved = set(rows_big.values())
    deal = 0
    for s in range(S):
        pv = plant_values(edges[:, s]) + [("test0", None), ("both0", None)]
        pv[[n for n, _ in pv].index("far")] = ("far", FAR + s)
        lane, last_lane = s % 64, min(63, S - 1 - 64 * (s // 64))
        free = [r for r in rng.permutation(E) if int(r) not in reserved]
        if placed:
            assert len(free) >= len(pv)
        if len(free) < len(pv):                   # fewer rows than plants: deal them round the samples
            pv = [pv[(deal + i) % len(pv)] for i in range(len(free))]
            deal += len(free)
        for name, v in pv:
            if placed and name in BIG_NAMES:
                row = rows_big[{"rtab": "all_a", "rtab+1": "all_b", "far": "all_far"}[name]]
                if name == "rtab" and lane == 0:
                    row = rows_big["first_lane"]
                if name == "rtab" and lane == last_lane and lane != 0:
                    row = rows_big["last_lane"]
                if name == "rtab+1" and lane == 31:
                    row = rows_big["last_row"]
                if name == "far" and lane == 0:
                    row = rows_big["walk_end"]
                if name == "rtab+1" and lane == 1 and "second_wg" in rows_big:
                    row = rows_big["second_wg"]
            else:
                row = int(free.pop())
            if name == "test0":
                test[row, s] = 0
                ref[row, s] = max(ref[row, s], 1)
            elif name == "both0":
                test[row, s] = 0; ref[row, s] = 0
            else:
                ref[row, s] = v
                test[row, s] = max(_test_for(v, expected[s], rng), 1) if name == "zero" else _test_for(v, expected[s], rng)
            planted[s][name] = row
    if placed:
        # nothing but the plants reaches the table's end
        keep = np.zeros((E, S), dtype=bool)
        for s in range(S):
            for n in BIG_NAMES:
                keep[planted[s][n], s] = True
        assert np.all((ref < RTAB) | keep)
    assert ref.min() >= 0 and test.min() >= 0 and (ref + test).max() < 2 ** 31
    return {"E": E, "S": S, "B": B, "sizes": tuple(sizes), "chrom_off": chrom_off, "start": start, "end": end, "test": test.astype(np.int32),
            "ref": ref.astype(np.int32), "phi_bins": phi_bins, "edges": edges, "expected": expected, "planted": planted, "placed": placed,
            "ood_sample": ood_sample}


def bins_fold_case(seed=7):
    """E = 262 145: 65 537 exon blocks, one more than two grid folds of 65 535 hold in y; counts >= RTAB in the first and the last block"""
    E, S, B, sizes = FOLD_SHAPE
    rng = np.random.default_rng([seed, 14])
    chrom_off, start, end = design(sizes, seed)
    phi_bins, edges, expected = bins_params(S, B, seed)
    test, ref = _counts(E, S, edges, expected, rng)
    rows = (0, 3, 4 * 65535 + 1, E - 1)      # block 0, block 65535 (the first of z = 1), block 65536 (the last: one exon)
    for s in range(S):
        for i, r in enumerate(rows):
            ref[r, s] = (RTAB, RTAB + 1, FAR, FAR + 1)[(i + s) % 4]
            test[r, s] = _test_for(ref[r, s], expected[s], rng)
    return {"E": E, "S": S, "B": B, "sizes": sizes, "chrom_off": chrom_off, "start": start, "end": end, "test": test.astype(np.int32),
            "ref": ref.astype(np.int32), "phi_bins": phi_bins, "edges": edges, "expected": expected, "big_rows": rows, "placed": False,
            "ood_sample": None}


def mixtures(S):
    """distinct per-sample mixtures in (0.2, 1.0]"""
    return 0.2 + 0.8 * (np.arange(S) + 1.0) / S


def tile_census(case):
    """cells a sample leaves to the per-cell kernel by its reference count alone, per (exon block, sample block) tile: [eblk][gx]"""
    E, S = case["E"], case["S"]
    eblk, gx = (E + TILE_ROWS - 1) // TILE_ROWS, (S + 63) // 64
    big = case["ref"] >= RTAB
    n = np.zeros((eblk, gx), dtype=np.int64)
    for e, s in zip(*np.nonzero(big)):
        n[e // TILE_ROWS, s // 64] += 1
    return big, n


# ---------------------------------------------------------------------------------------------------------------------------
# covariates
# ---------------------------------------------------------------------------------------------------------------------------
def cov_restate_expected(X, beta, pexp):
    """cov_expected (csrc/edcore.hip) in float64 with the device's order of operations: eta = beta0; eta += beta[k+1] * x[k], k ascending;
    1 / (1 + pexp(-eta)).  pexp: the checker's portable exp (oracle.pexp).  (E, S)"""
    E, K = X.shape
    S = beta.shape[1]
    eta = np.repeat(beta[0][None, :], E, axis=0).astype(np.float64)
    for k in range(K):
        eta = eta + beta[k + 1][None, :] * X[:, k][:, None]
    return 1.0 / (1.0 + pexp(-eta.ravel()).reshape(E, S)), eta


def cov_emit_case(E, S, K, sizes, seed):
    """hand-set beta (K + 1, S) and phi (S); X (E, K) with rows of zeros, repeated rows and rows that carry X.beta to both ends of
    [-20, 20] (the first covariate spans [-1, 1] and some samples have a slope of 17 on it)"""
    assert sum(sizes) == E
    rng = np.random.default_rng([seed, 15])
    chrom_off, start, end = design(sizes, seed)
    X = np.stack([rng.uniform(-1, 1, E), rng.normal(0.0, 1.0, E), rng.uniform(0.3, 0.7, E) - 0.5], axis=1)[:, :K]
    if K and E >= 3:
        X[0] = 0.0                                    # a row of zeros
        X[E - 1] = X[1]                               # a repeated row
    if K and E >= 5:
        X[2, 0] = 1.0; X[3, 0] = -1.0                 # the ends of the first covariate
        if K > 1:
            X[2, 1:] = 0.0; X[3, 1:] = 0.0
    X = np.ascontiguousarray(X, dtype=np.float64)
    beta = np.zeros((K + 1, S))
    beta[0] = rng.uniform(-2.6, -0.4, S)
    if K >= 1:
        beta[1] = np.where(np.arange(S) % 3 == 0, np.sign(rng.uniform(-1, 1, S)) * 17.0, rng.uniform(-1.6, 1.6, S))
    if K >= 2:
        beta[2] = rng.uniform(-0.15, 0.15, S)
    if K >= 3:
        beta[3] = rng.uniform(-0.3, 0.3, S)
    phi = rng.uniform(0.002, 0.008, S)
    eta = beta[0][None, :] + X @ beta[1:]
    p = 1.0 / (1.0 + np.exp(-eta))
    tot = rng.poisson(rng.lognormal(np.log(300.0), 0.6, E))[:, None] + rng.integers(0, 40, (E, S))
    test = rng.binomial(tot, p)
    if E >= 12:
        for s in range(S):
            for rep in range(max(1, E // 120)):
                a = int(rng.integers(0, E - 10)); n = int(rng.integers(6, 11))
                test[a:a + n, s] = np.minimum(np.floor(test[a:a + n, s] * (0.5 if (s + rep) % 2 else 1.5)), tot[a:a + n, s])
    ref = tot - test
    if E >= 3:
        for s in range(S):
            r = rng.permutation(E)[:2]
            ref[r[0], s] += test[r[0], s]; test[r[0], s] = 0          # test = 0
            test[r[1], s] = 0; ref[r[1], s] = 0                        # test = ref = 0
    assert test.min() >= 0 and ref.min() >= 0
    return {"E": E, "S": S, "K": K, "sizes": tuple(sizes), "chrom_off": chrom_off, "start": start, "end": end, "X": X, "beta": beta, "phi": phi,
            "test": test.astype(np.int32), "ref": ref.astype(np.int32)}


# ---------------------------------------------------------------------------------------------------------------------------
# fits
# ---------------------------------------------------------------------------------------------------------------------------
# (E, S, B, form): every E and every S once per form; B = 2, 3 run k_lh_hist<4>, B = 4, 7 k_lh_hist<2>, B = 8 k_lh_hist<1>, each at an S
# that is no multiple of its samples per workgroup; no S is a multiple of k_lh_rhist's 8.  4097 exons are 20 sub-chunks (> kRedY = 16);
# (261 - 1) * 0.85 and (1021 - 1) * 0.85 are integers in double arithmetic, the other (E - 1) * 0.85 are not.
FIT_BINS = ((255, 1, 2, 1), (256, 7, 3, 1), (257, 9, 4, 1), (1023, 63, 7, 1), (1025, 65, 8, 1), (4097, 130, 3, 1), (261, 9, 2, 1),
            (255, 65, 2, 0), (256, 130, 3, 0), (257, 1, 4, 0), (1023, 9, 8, 0), (1025, 7, 7, 0), (4097, 63, 4, 0), (1021, 9, 3, 0))
# (E, S, K)
FIT_COV = ((255, 1, 1), (256, 7, 0), (257, 9, 2), (1023, 63, 3), (1025, 65, 1), (4097, 130, 2))


def check_cols(S):
    """the columns whose estimates are compared with the checker: the first and last of every 64-lane block (dead lanes follow the
    last), and the neighbours of the 4- and 8-sample workgroups of the histogram kernels"""
    c = {0, 1, 3, 4, 7, 8, 62, 63, 64, 65, 127, 128, S - 2, S - 1}
    return sorted(x for x in c if 0 <= x < S)


def fit_bins_case(E, S, B, seed, depth=1500.0, tie_col=None):
    """counts for fit_bins: reference depths spread evenly over the levels (complete.bins cuts [0, q85] into B - 1 equal parts), true
    dispersions 0.01 .. 0.05 so that every level's estimate is well inside (1e-3, 0.1).  tie_col: a column whose reference counts of
    rank 0.80 E .. 0.90 E are all equal -- the two order statistics of the 0.85 quantile coincide."""
    rng = np.random.default_rng([seed, 16])
    test = np.zeros((E, S), dtype=np.int64); ref = np.zeros((E, S), dtype=np.int64)
    for s in range(S):
        p = rng.uniform(0.15, 0.45)
        phi = rng.uniform(0.01, 0.05)
        tot = rng.poisson(rng.uniform(0.02, 1.0, E) * depth * rng.uniform(0.7, 1.3))
        pp = rng.beta(p * (1 - phi) / phi, (1 - p) * (1 - phi) / phi, E)
        y = rng.binomial(tot, pp)
        test[:, s] = y; ref[:, s] = tot - y
    if tie_col is not None:
        o = np.argsort(ref[:, tie_col], kind="stable")
        a, b, m = int(0.80 * E), int(0.90 * E), int(0.85 * E)
        ref[o[a:b], tie_col] = ref[o[m], tie_col]
    return test.astype(np.int32), ref.astype(np.int32)


def fit_bins_args(i):
    E, S, B, form = FIT_BINS[i]
    return dict(E=E, S=S, B=B, seed=900 + i, tie_col=min(1, S - 1))


def fit_cov_case(E, S, K, seed, depth=200.0):
    """as tests/test_gpu_cov.py's cohort: covariates of the size of GC content / exon length effects, dispersions 0.003 .. 0.012"""
    rng = np.random.default_rng([seed, 17])
    X = np.ascontiguousarray(np.stack([rng.uniform(0.3, 0.7, E) - 0.5, rng.normal(0.0, 1.0, E), rng.uniform(-1, 1, E)], axis=1)[:, :K])
    lam = rng.lognormal(np.log(depth), 0.6, E)
    test = np.zeros((E, S), dtype=np.int32); ref = np.zeros((E, S), dtype=np.int32)
    for s in range(S):
        beta = np.concatenate([[rng.uniform(-2.4, -1.6)], rng.uniform(-0.8, 0.8, K) * np.array([2.0, 0.15, 0.3])[:K]])
        phi = rng.uniform(0.003, 0.012)
        p = 1 / (1 + np.exp(-(beta[0] + X @ beta[1:])))
        tot = rng.poisson(lam * 9)
        y = rng.binomial(tot, rng.beta(p * (1 - phi) / phi, (1 - p) * (1 - phi) / phi))
        test[:, s] = y; ref[:, s] = tot - y
    return X, test, ref


# the histogram form's limits (csrc/edbins_hist.inc)
LH_BINS = 8192          # kLhKq: unit bins of the reference count
LH_LIST = 32768         # kLhListTotal
LH_KY = 1024            # kLhKy: unit bins of the test count


def quantile_ranks(E):
    """0-based ranks (k0, k1) of the two order statistics of quantile(., 0.85), type 7, and the weight h of the upper one"""
    index = 1.0 + max(E - 1, 0) * 0.85
    lo, hi = int(np.floor(index)), int(np.ceil(index))
    return lo - 1, hi - 1, index - lo


def quantile_edge_case(outside, seed=31, E=400, S=3):
    """reference counts whose upper order statistic of the 0.85 quantile (rank k1) is the LAST count inside the 8192 unit bins (8191, with
    exactly k1 + 1 counts below 8192: k_lh_select finds it) or, in column 1 of the `outside` case, the first one beyond them (exactly k1
    counts below 8192: the rank is not inside the bins and the form declines)"""
    rng = np.random.default_rng([seed, 18])
    k0, k1, h = quantile_ranks(E)
    test = np.zeros((E, S), dtype=np.int64); ref = np.zeros((E, S), dtype=np.int64)
    for s in range(S):
        inside = k1 + 1 - (1 if (outside and s == 1) else 0)
        low = np.sort(rng.integers(40, LH_BINS - 200, inside))
        if not (outside and s == 1):
            low[-1] = LH_BINS - 1
        high = rng.integers(LH_BINS, 12000, E - inside)
        r = np.concatenate([low, high])[rng.permutation(E)]
        p = rng.uniform(0.05, 0.10); phi = rng.uniform(0.01, 0.04)
        tot = np.floor(r / (1 - p)).astype(np.int64)
        y = rng.binomial(tot, rng.beta(p * (1 - phi) / phi, (1 - p) * (1 - phi) / phi, E))
        test[:, s] = y; ref[:, s] = r
    return test.astype(np.int32), ref.astype(np.int32)


def list_overflow_case(seed=32, E=40000):
    """one sample, reference counts inside the bins, test counts >= 1024 on most rows: more than 32 768 cells outside their y bins"""
    rng = np.random.default_rng([seed, 19])
    p, phi = 0.42, 0.02
    tot = rng.poisson(rng.uniform(0.3, 1.0, E) * 9000.0)
    y = rng.binomial(tot, rng.beta(p * (1 - phi) / phi, (1 - p) * (1 - phi) / phi, E))
    return y.astype(np.int32)[:, None], (tot - y).astype(np.int32)[:, None]


def range_case(seed=33, E=600, S=3):
    """an ordinary batch with one test count of 2^28 in column 1"""
    test, ref = fit_bins_case(E, S, 3, seed)
    test = test.copy()
    test[E // 2, 1] = 1 << 28
    return test, ref


# ---------------------------------------------------------------------------------------------------------------------------
# cohort slabs
# ---------------------------------------------------------------------------------------------------------------------------
COHORT_SLAB = 65


def cohort_case(E, n_slabs=3, seed=41):
    """slabs of 65 samples for Cohort(..., phi_bins = 3).  At E = 6 the reference counts are spread so that the three depth levels
    (edges 0, q85 / 2, q85) are populated in every sample."""
    rng = np.random.default_rng([seed, 20, E])
    sizes = (E,) if E < 20 else (E // 3, E - E // 3)
    chrom_off, start, end = design(sizes, seed)
    slabs = []
    for i in range(n_slabs):
        if E < 20:
            base = np.array([100, 300, 600, 700, 800, 1000] + [900] * (E - 6))[:E]
            ref = np.floor(base[rng.permutation(E)][:, None] * rng.uniform(0.9, 1.1, (E, COHORT_SLAB))).astype(np.int64)
            p = rng.uniform(0.2, 0.4, COHORT_SLAB)
            test = rng.binomial(np.floor(ref / (1 - p[None, :])).astype(np.int64), p[None, :])
        else:
            test, ref = fit_bins_case(E, COHORT_SLAB, 3, seed + 10 * i, depth=400.0)
            test = test.astype(np.int64); ref = ref.astype(np.int64)
            for s in range(COHORT_SLAB):
                a = int(rng.integers(0, E - 8)); n = int(rng.integers(4, 9))
                test[a:a + n, s] = np.floor(test[a:a + n, s] * (0.5 if s % 2 else 1.5))
            # a few reference counts beyond the table of constants, in the first and the last exon block
            ref[0, i] = RTAB; ref[E - 1, (i + 7) % COHORT_SLAB] = RTAB + 1 + i
        slabs.append((test.astype(np.int32), ref.astype(np.int32)))
    return chrom_off, start, end, slabs
