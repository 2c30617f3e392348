"""tests/test_gpu_emit_geometry.py's inputs without a GPU: the generators of tests/emit_geometry_cases.py are deterministic, and every
case is what the GPU tests take it for -- judged on the CPU, from the arrays and by the checker alone."""
import numpy as np
import pytest

import emit_geometry_cases as gc
import test_gpu_emit_geometry as tg


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))


def test_generators_are_deterministic():
    E, S, B, sizes = gc.BINS_SHAPES[4]
    a = gc.bins_emit_case(E, S, B, sizes, 5)
    assert _same(a, gc.bins_emit_case(E, S, B, sizes, 5)) and a["planted"] == gc.bins_emit_case(E, S, B, sizes, 5)["planted"]
    assert not np.array_equal(a["ref"], gc.bins_emit_case(E, S, B, sizes, 6)["ref"])
    E, S, K, sizes = gc.COV_SHAPES[2]
    c = gc.cov_emit_case(E, S, K, sizes, 5)
    assert _same(c, gc.cov_emit_case(E, S, K, sizes, 5)) and not np.array_equal(c["test"], gc.cov_emit_case(E, S, K, sizes, 6)["test"])
    for f, args in ((gc.fit_bins_case, (300, 5, 3, 1)), (gc.fit_cov_case, (300, 5, 2, 1)), (gc.quantile_edge_case, (True,)),
                    (gc.list_overflow_case, ()), (gc.range_case, ())):
        x, y = f(*args), f(*args)
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert not np.array_equal(gc.fit_bins_case(300, 5, 3, 1)[1], gc.fit_bins_case(300, 5, 3, 2)[1])
    x, y = gc.cohort_case(6), gc.cohort_case(6)
    assert all(np.array_equal(p[1], q[1]) and np.array_equal(p[0], q[0]) for p, q in zip(x[3], y[3]))


def test_bins_shapes_cover_what_the_sweep_promises():
    assert [s[:2] for s in gc.BINS_SHAPES] == [(1, 1), (3, 65), (4, 64), (5, 63), (130, 130), (258, 2), (1027, 65)]
    assert sorted(s[2] for s in gc.BINS_SHAPES) == [2, 3, 4, 5, 6, 7, 8]
    assert all(1 <= len(s[3]) <= 3 and sum(s[3]) == s[0] for s in gc.BINS_SHAPES) and any(0 in s[3] for s in gc.BINS_SHAPES)
    E, S, B, sizes = gc.FOLD_SHAPE
    assert (E + 3) // 4 == 65537 and S == 2 and len(sizes) == 4 and sum(sizes) == E


@pytest.mark.parametrize("idx", range(len(gc.BINS_SHAPES)))
def test_planted_reference_counts(oracle, idx):
    """every plant is where the record says, and the plants land on the branches they are meant for (decided by the checker's
    approx_linear and by the table's end)"""
    from oracle import bins_oracle as bo
    case = tg.bins_case(idx)
    E, S, B = case["E"], case["S"], case["B"]
    test, ref, edges = case["test"], case["ref"], case["edges"]
    assert test.dtype == np.int32 and ref.dtype == np.int32 and test.min() >= 0 and ref.min() >= 0
    seen = set()
    for s in range(S):
        mid = gc.midpoints(edges[:, s])
        assert np.all(np.diff(mid) > 2) and np.all(np.diff(edges[:, s]) > 0) and edges[0, s] == 0
        names = [n for n, _ in gc.plant_values(edges[:, s])] + ["test0", "both0"]
        pl = case["planted"][s]
        if E >= 130:
            assert sorted(pl) == sorted(names), s                    # every sample contains all of them
            assert len(set(pl.values())) == len(pl)
        values = dict(gc.plant_values(edges[:, s]))
        values["far"] = gc.FAR + s
        for n, row in pl.items():
            seen.add(n)
            if n == "test0":
                assert test[row, s] == 0 and ref[row, s] > 0
            elif n == "both0":
                assert test[row, s] == 0 and ref[row, s] == 0
            else:
                assert ref[row, s] == values[n], (s, n)
        if E >= 130:
            v = ref[:, s].astype(np.float64)
            assert (v < mid[0]).any() and (v > mid[-1]).any() and (ref[:, s] == 0).any()
            for g, m in enumerate(mid):
                if m == np.floor(m):
                    assert {int(m) - 1, int(m), int(m) + 1} <= set(ref[:, s].tolist())
                else:
                    assert {int(np.floor(m)), int(np.ceil(m))} <= set(ref[:, s].tolist())
            if s % 4 != 3:
                assert (mid[:-1] == np.floor(mid[:-1])).all() and mid[-1] != np.floor(mid[-1])
            else:
                assert (mid[:-1] != np.floor(mid[:-1])).all()
            for k in range(B + 1):
                assert int(np.floor(edges[k, s])) in set(ref[:, s].tolist())
            assert {gc.RTAB - 1, gc.RTAB, gc.RTAB + 1, gc.FAR + s} <= set(ref[:, s].tolist())
            assert ((test[:, s] == 0) & (ref[:, s] > 0)).any() and ((test[:, s] == 0) & (ref[:, s] == 0)).any()
            assert ((test[:, s] > 0) & (ref[:, s] == 0)).any()
            # approx_linear returns y[j] exactly on an integer mid-point, yleft / yright outside
            y = case["phi_bins"][:, s]
            ints = [g for g in range(B) if mid[g] == np.floor(mid[g])]
            if ints:
                assert np.array_equal(bo.approx_linear(mid[ints], mid, y), y[ints])
    if E * S >= 60:
        assert {"zero", "below", "above", "rtab-1", "rtab", "rtab+1", "far", "test0", "both0", "edge0", "edge%d" % B} <= seen
        assert any(n.startswith("mid0") for n in seen) and any(n.startswith("mid%d" % (B - 1)) for n in seen)
    # a finite checker result everywhere: the bit-for-bit comparison has no NaN to excuse
    want = tg.bins_expect(oracle, case, ("shape", idx))
    assert np.all(np.isfinite(want["ll"])) and want["nerr"].sum() == 0
    if E >= 130:
        assert sum(len(c) for c in want["calls"]) > 0


@pytest.mark.parametrize("idx", [4, 5])
def test_tile_placement_of_the_counts_beyond_the_table(idx):
    case = tg.bins_case(idx)
    E, S = case["E"], case["S"]
    assert case["placed"] and E in (130, 258)
    big, n = gc.tile_census(case)
    eblk, gx = n.shape
    assert eblk == (33 if E == 130 else 65) and eblk % gc.TILES_PER_WG == 1          # a partial last workgroup of one tile
    assert (n == 0).sum() >= eblk * gx // 2                                           # most tiles have none
    rows = gc.big_rows(E)
    once = [(t, bx) for t, bx in np.argwhere(n == 1)]

    def cell(t, bx):
        e, s = np.argwhere(big[t * 4:t * 4 + 4, bx * 64:bx * 64 + 64])[0]
        return int(e), int(s)
    where = {(t, bx): cell(t, bx) for t, bx in once}
    assert (0, 0) in where.values()                                                   # exactly one, at the tile's first lane
    assert any(v[0] == 3 for v in where.values())                                     # exactly one, in the tile's last exon row
    last_lane = min(63, S - 1)
    assert (3, last_lane) in [where.get((rows["last_lane"] // 4, bx)) for bx in range(gx)]   # exactly one, at the last lane of the tile
    wg = np.add.reduceat((n > 0).astype(int), np.arange(0, eblk, gc.TILES_PER_WG), axis=0)   # non-empty tiles per 32-tile workgroup
    assert (wg[0] >= 2).all() and (wg[-1] >= 1).any()
    assert (n[gc.TILES_PER_WG - 1] > 0).any()                                         # the last tile of a workgroup's walk
    assert big[E - 1].any()                                                           # the last exon row of the matrix
    if S > 64:
        assert (n[:, 1:] > 0).any()                                                   # left_out is indexed blk * gx + bx with bx > 0


def test_out_of_domain_sample(oracle):
    case = tg.bins_case(4, ood_sample=70)
    want = tg.bins_expect(oracle, case, ("ood", 4), calls=False)
    nan = np.isnan(want["ll"])
    assert want["nerr"].sum() > 0 and want["nerr"][70] == want["nerr"].sum()
    assert nan[:, :, 70].any() and not nan[:, :, :70].any() and not nan[:, :, 71:].any()
    assert np.isfinite(want["ll"][:, :, 70]).sum() > want["ll"][:, :, 70].size // 4  # and most of that sample still carries values


def test_fold_case():
    case = tg.cached(("fold",), gc.bins_fold_case)
    E = case["E"]
    blocks = sorted(set(r // 4 for r in case["big_rows"]))
    assert blocks[0] == 0 and blocks[-1] == 65536 and 65535 in blocks
    assert all((case["ref"][r] >= gc.RTAB).all() for r in case["big_rows"])
    assert len(case["chrom_off"]) == 5 and case["chrom_off"][-1] == E


def test_mixtures():
    for S in (63, 130):
        m = gc.mixtures(S)
        assert len(set(m.tolist())) == S and m.min() > 0.2 and m.max() == 1.0


@pytest.mark.parametrize("idx", range(len(gc.COV_SHAPES)))
def test_covariate_cases(oracle, idx):
    case = tg.cov_case(idx)
    E, S, K, X = case["E"], case["S"], case["K"], case["X"]
    assert X.shape == (E, K) and case["beta"].shape == (K + 1, S)
    expd, eta = gc.cov_restate_expected(X, case["beta"], oracle.pexp)
    assert np.all((expd > 0) & (expd < 1)) and np.abs(eta).max() <= 20.0
    if K and E >= 5:
        assert not X[0].any() and np.array_equal(X[E - 1], X[1])
        assert eta.min() < -15.0 and eta.max() > 12.0                                 # X.beta reaches both ends of [-20, 20]
    assert np.allclose(expd, 1 / (1 + np.exp(-eta)), rtol=1e-14, atol=0)
    want = tg.cov_expect(oracle, case, idx)
    assert np.all(np.isfinite(want["ll"]))
    assert ((case["test"] == 0) & (case["ref"] > 0)).any() and ((case["test"] == 0) & (case["ref"] == 0)).any()
    if E >= 130:
        assert sum(len(c) for c in want["calls"]) > 0
    assert sorted(s[2] for s in gc.COV_SHAPES) == [0, 1, 2, 3]


def test_fit_grids():
    for form in (0, 1):
        rows = [c for c in gc.FIT_BINS if c[3] == form]
        assert {c[0] for c in rows} >= {255, 256, 257, 1023, 1025, 4097} and {c[1] for c in rows} == {1, 7, 9, 63, 65, 130}
    assert {c[2] for c in gc.FIT_BINS} == {2, 3, 4, 7, 8}
    for E, S, B, form in gc.FIT_BINS:
        if form == 1:
            ks = 4 if B <= 3 else 2 if B <= 7 else 1
            assert ks == 1 or S % ks != 0
            assert S % 8 != 0
    assert {c[0] for c in gc.FIT_COV} == {255, 256, 257, 1023, 1025, 4097} and {c[1] for c in gc.FIT_COV} == {1, 7, 9, 63, 65, 130}
    assert {c[2] for c in gc.FIT_COV} == {0, 1, 2, 3}
    whole = {E: float((E - 1) * 0.85).is_integer() for E in {c[0] for c in gc.FIT_BINS}}
    assert whole[261] and whole[1021] and not whole[255] and not whole[4097] and sum(whole.values()) == 2
    assert (4097 + 255) // 256 > 16                                                   # more sub-chunks than kRedY


@pytest.mark.parametrize("i", range(len(gc.FIT_BINS)))
def test_fit_bins_preconditions(oracle, i):
    from oracle import bins_oracle as bo
    E, S, B, form = gc.FIT_BINS[i]
    args = gc.fit_bins_args(i)
    test, ref = gc.fit_bins_case(**args)
    assert test.shape == (E, S)
    k0, k1, h = gc.quantile_ranks(E)
    tie = args["tie_col"]
    x = np.sort(ref[:, tie])
    assert x[k0] == x[k1]                                                             # the two order statistics coincide
    if S > 1:
        x = np.sort(ref, axis=0)
        assert (x[k0] != x[k1]).any() or k0 == k1                                     # ... and in other columns they do not
    for s in range(S):
        bo.depth_bins(ref[:, s], B)                                                   # raises when a level is empty
    for s in gc.check_cols(S):
        ophi, op, _, _ = bo.fit_bins(test[:, s], ref[:, s], B)
        assert np.all((ophi >= 1e-3) & (ophi <= 0.1)), (E, S, B, s, ophi)


def test_some_column_needs_the_clamp_of_the_last_edge():
    """seq(0, q, by = q / (B - 1)) ends in pmin(., q): in some column of the fit cases (B - 1) * by exceeds q in double arithmetic"""
    n = 0
    for i, (E, S, B, form) in enumerate(gc.FIT_BINS):
        test, ref = gc.fit_bins_case(**gc.fit_bins_args(i))
        k0, k1, h = gc.quantile_ranks(E)
        x = np.sort(ref, axis=0).astype(np.float64)
        q = np.where((h > 0) & (x[k1] != x[k0]), (1.0 - h) * x[k0] + h * x[k1], x[k0])
        n += int(((B - 1) * (q / (B - 1)) > q).sum())
    assert n > 0


@pytest.mark.parametrize("i", range(len(gc.FIT_COV)))
def test_fit_cov_preconditions(oracle, i):
    E, S, K = gc.FIT_COV[i]
    X, test, ref = gc.fit_cov_case(E, S, K, 950 + i)
    for s in gc.check_cols(S):
        _, ophi, _, _ = oracle.fit_mle_cov(test[:, s], ref[:, s], X)
        assert 1e-4 < ophi < 0.1, (E, S, K, s, ophi)


def test_histogram_form_limit_cases(oracle):
    from oracle import bins_oracle as bo
    for outside in (False, True):
        test, ref = gc.quantile_edge_case(outside)
        E, S = ref.shape
        k0, k1, h = gc.quantile_ranks(E)
        inside = (ref < gc.LH_BINS).sum(axis=0)
        assert inside.tolist() == [k1 + 1, k1 + (0 if outside else 1), k1 + 1]
        x = np.sort(ref, axis=0)
        assert x[k1, 0] == gc.LH_BINS - 1 and x[k1, 2] == gc.LH_BINS - 1 and (x[k1, 1] >= gc.LH_BINS) == outside
        for s in range(S):
            ophi = bo.fit_bins(test[:, s], ref[:, s], 3)[0]
            assert np.all((ophi >= 1e-3) & (ophi <= 0.1))
    test, ref = gc.list_overflow_case()
    assert test.shape == (40000, 1) and ref.max() < gc.LH_BINS
    assert ((test[:, 0] >= gc.LH_KY) & (test[:, 0] + ref[:, 0] > 0)).sum() > gc.LH_LIST
    ophi = bo.fit_bins(test[:, 0], ref[:, 0], 3)[0]
    assert np.all((ophi >= 1e-3) & (ophi <= 0.1))
    test, ref = gc.range_case()
    assert (test >= 1 << 28).sum() == 1 and test[:, 1].max() == 1 << 28 and ref.max() < gc.LH_BINS
    assert int(test.max()) + int(ref.max()) < 2 ** 31
    for s in range(test.shape[1]):
        bo.fit_bins(test[:, s], ref[:, s], 3)


@pytest.mark.parametrize("E", [6, 130])
def test_cohort_slabs(E):
    from oracle import bins_oracle as bo
    chrom_off, start, end, slabs = gc.cohort_case(E)
    assert len(slabs) == 3 and (E + 3) // 4 == (2 if E == 6 else 33)
    for test, ref in slabs:
        assert test.shape == (E, gc.COHORT_SLAB) and test.min() >= 0 and ref.min() >= 0
        for s in range(gc.COHORT_SLAB):
            bo.depth_bins(ref[:, s], 3)                                               # every level populated
        if E == 130:
            assert (ref[0] >= gc.RTAB).any() and (ref[E - 1] >= gc.RTAB).any()
