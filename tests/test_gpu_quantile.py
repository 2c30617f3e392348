"""The quantile map on the GPU (csrc/edquant.inc) against the 40-digit checker (tests/quantile_checker.py) in probability space, at crossings
planted on the walk's edges, bit for bit against itself, through the element-wise entry, at the edges of its occupancy map and of its
region records, and through the Python surface.

A device pair (q, below) for (n, a, b, p) is judged by quantile_checker.judge: |G(q) - p| <= bar, where G is the piecewise-linear function
q inverts, and below = C(x - 1) within the bar for a value x that is a cut of p within the bar; a NaN must have 1 - p within the bar.
G is continuous in the masses, so no case stands next to a threshold and none is excused.  The bar is derived from the walk's own
operations (quantile_checker.bar), not from what the device returns.
Figures measured on an MI355X when this file was written (the tests print them with -s): DESIGN.md 4.24.
"""
import ctypes as C
import math

import numpy as np
import pytest

import quantile_checker as qc

pytestmark = pytest.mark.gpu

PHIS = (1e-5, 0.003, 0.05, 0.2)
EXPECTED = (0.05, 0.11, 0.4)
PROB_LISTS = ((0.025, 0.975), (0.5,), (1e-4, 1.0 - 1e-4),
              (1e-4, 0.001, 0.01, 0.025, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.975, 0.99, 1.0 - 1e-4))
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def design(sizes, step=1000, width=120):
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    start = np.concatenate([np.arange(m, dtype=np.int64) * step + 1 for m in sizes] + [np.zeros(0, np.int64)]).astype(np.int32)
    return chrom_off, start, (start + width).astype(np.int32)


def make_map(edlib, sizes, test, ref, phi, expected, probs=(0.025, 0.975), layout=0, device=False):
    """test, ref: (E, S) int32"""
    chrom_off, start, end = design(sizes)
    plan = edlib.Plan(chrom_off, start, end)
    test, ref = np.ascontiguousarray(test, dtype=np.int32), np.ascontiguousarray(ref, dtype=np.int32)
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    if device:
        test, ref = edlib.DeviceArray(test), edlib.DeviceArray(ref)
    qm = plan.quantile_map(test, ref, phi, expected, probs, layout=layout)
    if device:
        test.free()
        ref.free()
    return plan, qm


def totals_map(edlib, totals, phi, expected, probs):
    """every sample sees every total once; the totals are all in the reference count"""
    tot = np.repeat(np.asarray(totals, dtype=np.int32)[:, None], len(phi), axis=1)
    return make_map(edlib, [len(totals)], np.zeros_like(tot), tot, phi, expected, probs)


def edge_totals(edlib):
    g = edlib.quantile_geometry()
    assert g["walk_tile"] == 256 and g["occupancy_cap"] == 32768
    return [0, 1, 2, 3, 5, 17, 63, 64, 255, 256, 257, 511, 512, 513, 600, 1025, 4099, g["occupancy_cap"] + 1]


def _edge_tables(edlib):
    if "edge" not in _CACHE:
        totals = edge_totals(edlib)
        par = [(p, e) for p in PHIS for e in EXPECTED]
        out = {}
        for probs in PROB_LISTS:
            plan, qm = totals_map(edlib, totals, [q[0] for q in par], [q[1] for q in par], probs)
            out[probs] = ([qm.table(s) for s in range(len(par))], qm.stats())
            qm.free()
            plan.close()
        _CACHE["edge"] = (totals, par, out)
    return _CACHE["edge"]


# ---- 1. the walk's edges against the checker ---------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", PHIS)
def test_walk_edges_against_the_checker(edlib, phi):
    totals, par, out = _edge_tables(edlib)
    worst, n_cases = 0.0, 0
    for probs in PROB_LISTS:
        tabs, st = out[probs]
        assert st["n_bad_samples"] == 0 and st["n_skipped"] == 0 and st["n_jobs"] == len(totals) * len(par) and st["n_probs"] == len(probs)
        assert st["map_words"] == edlib.quantile_geometry()["max_total"] // 32 + 1          # one total above the narrow map's cap
        for s, (ph, e) in enumerate(par):
            if ph != phi:
                continue
            a, b = qc.shapes(ph, e)
            t = tabs[s]
            assert list(t["totals"]) == sorted(totals)
            for j, n in enumerate(t["totals"]):
                for k, p in enumerate(probs):
                    q, bl = float(t["q"][k, j]), float(t["below"][k, j])
                    if n == 0:
                        assert q == p and bl == 0.0
                        continue
                    frac, tol = qc.judge(q, bl, int(n), a, b, p)
                    worst, n_cases = max(worst, frac), n_cases + 1
                    assert frac <= 1.0, (ph, e, int(n), p, q, bl, frac, tol)
                    assert q == q, (ph, e, int(n), p)              # at these probabilities the last mass is far above the bar: a crossing
    print("phi = %g: %d cases, largest fraction of the bar %.3g" % (phi, n_cases, worst))


def test_documented_examples_of_the_reference(edlib):
    """R/tools.R:17-18 and :40 through the element-wise entries, against the checker (tests/test_quantile_host.py says why not against R)"""
    got = [edlib.qbetabinom(0.2, 50, 0.4, 0.3), edlib.qbetabinom(0.2, 50, 0.1, 0.8), edlib.qbetabinom_ab(0.5, 50, 0.2, 0.25)]
    want = [(0.2, 50, qc.shapes(0.4, 0.3)), (0.2, 50, qc.shapes(0.1, 0.8)), (0.5, 50, (0.2, 0.25))]
    for g, (p, n, (a, b)) in zip(got, want):
        assert g.shape == (1,) and g.dtype == np.float64
        frac, _ = qc.judge(float(g[0]), None, n, a, b, p)
        print("q = %.15g (checker %.15g), fraction of the bar %.3g" % (g[0], float(qc.quantile(n, a, b, p)[0]), frac))
        assert frac <= 1.0


# ---- 2. planted crossings -----------------------------------------------------------------------------------------------------
def test_planted_crossings(edlib):
    worst = 0.0
    for name, n, phi, e, probs, cuts in qc.planted_cases():
        a, b = qc.shapes(phi, e)
        plan, qm = totals_map(edlib, [n], [phi], [e], probs)
        t = qm.table(0)
        qm.free()
        plan.close()
        assert list(t["totals"]) == [n]
        for k, (p, x) in enumerate(zip(probs, cuts)):
            q, bl = float(t["q"][k, 0]), float(t["below"][k, 0])
            frac, tol = qc.judge(q, bl, n, a, b, p)
            worst = max(worst, frac)
            assert frac <= 1.0, (name, p, q, bl, frac)
            if qc.margin(n, a, b, p, x) > 2 * tol:                 # p stands clear of its cell's ends: the cell is not in doubt
                assert q == q and qc.cut_of(q) == x and x < q < x + 1, (name, p, q, x)
                assert abs(bl - float(qc.below(n, a, b, x))) <= tol
                if x == 0:
                    assert bl == 0.0
            else:
                assert p == 1.0 - 2.0 ** -53, name                  # the one case planted within rounding of 1
                print("%s: q = %r, below = %r" % (name, q, bl))
        if name == "two in one cell":
            assert t["below"][0, 0] == t["below"][1, 0] and t["q"][0, 0] < t["q"][1, 0]
    # p >= 1 (the map refuses it; the element-wise entry takes it): NaN, R's NA
    assert np.all(np.isnan(edlib.qbetabinom_ab([1.0, 1.5, np.inf, np.nan], 17, 7.6, 11.4)))
    print("largest fraction of the bar %.3g" % worst)


# ---- 3. bit invariance --------------------------------------------------------------------------------------------------------
def _inv_case():
    rng = np.random.default_rng(41)
    sizes = [150, 0, 333, 70]
    E = sum(sizes)
    tot = rng.integers(0, 900, (E, 66)).astype(np.int32)
    tot[rng.choice(E, 9, replace=False), :] = 0
    test = rng.binomial(tot, 0.2).astype(np.int32)
    phi, e = rng.uniform(0.002, 0.05, 66), rng.uniform(0.08, 0.45, 66)
    rows = [(0, 0, 149), (0, 7, 7), (2, 150, 482), (2, 200, 290), (3, 483, 552), (3, 500, 552), (0, 60, 130)]
    return sizes, test, tot - test, phi, e, rows


def test_bit_invariance(edlib):
    sizes, test, ref, phi, e, rows = _inv_case()
    the = 33                                          # the sample that is followed through the settings
    others = [c for c in range(66) if c != the]
    probs = (0.025, 0.975)
    results = []
    for cols, layout, device in (([the], 0, False), ([the], 1, True), ([the, 1, 2], 0, True), ([1, the, 2], 1, False),
                                 (others[:63] + [the], 0, False), (others[:64] + [the], 1, True), ([the] + others[:64], 0, False)):
        assert len(cols) in (1, 3, 64, 65)
        at = cols.index(the)
        plan, qm = make_map(edlib, sizes, test[:, cols], ref[:, cols], phi[cols], e[cols], probs, layout=layout, device=device)
        order = list(range(len(rows))) if layout == 0 else [4, 2, 0, 6, 2, 1, 3, 5, 2]        # permuted and duplicated
        reg = qm.regions([rows[i] for i in order])
        first = {}
        for k, i in enumerate(order):
            if i in first:
                for key in ("observed", "expected", "n_empty", "chi2"):
                    assert reg[key][k, at].tobytes() == reg[key][first[i], at].tobytes()
            first.setdefault(i, k)
        pick = [first[i] for i in range(len(rows))]
        t = qm.table(at)
        results.append((t, qm.exons()[:, :, at, :], {k: np.ascontiguousarray(reg[k][pick, at]) for k in ("observed", "expected", "n_empty")}))
        qm.free()
        plan.close()
    t0, ex0, rg0 = results[0]
    assert t0["totals"].size > 100 and np.all(np.isfinite(ex0))
    for t, ex, rg in results[1:]:
        assert np.array_equal(t["totals"], t0["totals"]) and same_bits(t["q"], t0["q"]) and same_bits(t["below"], t0["below"]) and same_bits(ex, ex0)
        for k in rg0:
            assert rg[k].tobytes() == rg0[k].tobytes(), k
    # its probabilities alone or in a longer list: the bits of the shared ones
    for longer in ((0.025,), (0.975,), (0.001, 0.025, 0.5, 0.975), PROB_LISTS[3]):
        plan, qm = make_map(edlib, sizes, test[:, [the]], ref[:, [the]], phi[[the]], e[[the]], longer)
        ex = qm.exons()[:, :, 0, :]
        qm.free()
        plan.close()
        for k, p in enumerate(probs):
            if p in longer:
                assert same_bits(ex[:, longer.index(p)], ex0[:, k]), (longer, p)


# ---- 4. the element-wise entry --------------------------------------------------------------------------------------------------
def test_elementwise_entry(edlib):
    totals = [0, 1, 5, 63, 64, 255, 256, 257, 600, 1025]
    phi, e, probs = 0.003, 0.11, (0.025, 0.5, 0.975)
    plan, qm = totals_map(edlib, totals, [phi], [e], probs)
    t = qm.table(0)
    qm.free()
    plan.close()
    a, b = qc.shapes(phi, e)
    n = t["totals"].astype(np.float64)
    for k, p in enumerate(probs):
        assert same_bits(edlib.qbetabinom_ab(p, n, a, b), t["q"][k])
        assert same_bits(edlib.qbetabinom(p, n, phi, e), t["q"][k])
    # R's recycling: every argument to the longest
    r = edlib.qbetabinom_ab([0.025, 0.975], [600, 600, 257, 257], a, [b])
    assert r.shape == (4,)
    i600, i257 = list(t["totals"]).index(600), list(t["totals"]).index(257)
    assert same_bits(r, [t["q"][0, i600], t["q"][2, i600], t["q"][0, i257], t["q"][2, i257]])
    r = edlib.qbetabinom([0.5, 0.5, 0.5], 600, [phi, 0.05, phi], [e, e, 0.4])
    assert bits(r[0]) == bits(t["q"][1, i600]) and r[0] != r[1] and r[2] > r[0]
    assert edlib.qbetabinom_ab([], 5, 1.0, 1.0).shape == (0,)
    # what is no beta-binomial reads NaN; its neighbours do not notice
    top = edlib.quantile_geometry()["max_total"]
    r = edlib.qbetabinom_ab(0.5, [600, 600, 600, 600, 600, 2.5, -1, top + 1, 600], [a, 0.0, -1.0, np.inf, np.nan, a, a, a, a], b)
    assert bits(r[0]) == bits(t["q"][1, i600]) == bits(r[8]) and np.all(np.isnan(r[1:8]))
    assert np.all(np.isnan(edlib.qbetabinom_ab(0.5, 600, a, [0.0, -2.0, np.inf])))
    assert np.all(np.isnan(edlib.qbetabinom(0.5, 600, [1.0, 1.5, 0.0], e)))             # phi >= 1, phi = 0: no positive finite shapes
    assert edlib.qbetabinom(0.3, 0, phi, e)[0] == 0.3                                     # n = 0: q = p


# ---- 5. occupancy ---------------------------------------------------------------------------------------------------------------
def test_occupancy(edlib):
    g = edlib.quantile_geometry()
    top = g["max_total"]
    phi, e = [0.05, 1.0, 0.05, 1.5], [0.1, 0.1, 0.1, 0.1]
    ref = np.array([[12], [top], [77], [2], [77], [0], [top], [77]], np.int64).repeat(4, axis=1)
    test = np.zeros_like(ref)
    test[1, :], test[3, :], test[4, :] = 1, -5, 3          # exon 1: above the largest total; exon 3: a sum below 0; exon 4: 80
    plan, qm = make_map(edlib, [8], test, ref, phi, e, (0.025, 0.975))
    st, ex = qm.stats(), qm.exons()
    assert st["n_skipped"] == 2 * 4 and st["n_bad_samples"] == 2 and st["largest_total"] == top
    assert st["n_jobs"] == 4 * 5 and st["max_jobs"] == 5                    # 0, 12, 77 (three exons, walked once), 80, top
    assert np.all(np.isnan(ex[:, :, [1, 3], :])) and np.all(np.isnan(ex[:, :, :, [1, 3]]))
    assert np.all(np.isfinite(ex[:, :, [0, 2]][:, :, :, [0, 2, 4, 5, 6, 7]]))
    assert same_bits(ex[:, :, 0], ex[:, :, 2]) and same_bits(ex[:, :, 0, 2], ex[:, :, 0, 7])
    t = qm.table(0)
    assert list(t["totals"]) == [0, 12, 77, 80, top] and np.all(np.isnan(qm.table(1)["q"]))
    reg = qm.regions([(0, 0, 7)])
    assert list(reg["n_empty"][0]) == [2, 8, 2, 8] and np.all(reg["observed"][0, 1] == 0) and np.all(reg["expected"][0, 3] == 0.0)
    assert reg["observed"][0, 0].sum() == 6 and abs(reg["expected"][0, 0].sum() - 6.0) <= 6 * 2.0 ** -52
    qm.free()
    plan.close()
    a, b = qc.shapes(0.05, 0.1)
    for k, p in enumerate((0.025, 0.975)):
        for j, n in enumerate((12, 77, 80)):
            assert qc.judge(float(t["q"][k, j + 1]), float(t["below"][k, j + 1]), n, a, b, p)[0] <= 1.0
    # the batch-mates of a sample outside the model do not notice it
    plan, qm = make_map(edlib, [8], test[:, [0, 2]], ref[:, [0, 2]], [0.05, 0.05], [0.1, 0.1], (0.025, 0.975))
    assert qm.stats()["n_bad_samples"] == 0 and same_bits(qm.exons(), ex[:, :, [0, 2]])
    qm.free()
    plan.close()
    # the walk ends where its last probability is crossed
    n = 4099
    plan, qm = totals_map(edlib, [n], [0.003], [0.05], (0.025,))
    st = qm.stats()
    low = qm.table(0)
    qm.free()
    plan.close()
    full = -(-(n + 1) // g["walk_tile"])
    assert st["tiles_full"] == full == 17 and 1 <= st["tiles_walked"] < st["tiles_full"]
    assert st["tiles_walked"] == int(low["q"][0, 0]) // g["walk_tile"] + 1
    plan, qm = totals_map(edlib, [n], [0.003], [0.05], (0.025, 1.0 - 1e-12))
    st2, both = qm.stats(), qm.table(0)
    qm.free()
    plan.close()
    assert st["tiles_walked"] < st2["tiles_walked"] <= full and same_bits(both["q"][0], low["q"][0]) and same_bits(both["below"][0], low["below"][0])
    print("n = %d, p = 0.025 at expected 0.05: %d of %d tiles walked; with 1 - 1e-12: %d" % (n, st["tiles_walked"], full, st2["tiles_walked"]))


# ---- 6. regions -----------------------------------------------------------------------------------------------------------------
def test_regions(edlib):
    sizes = [130, 1, 65, 0, 64]
    rng = np.random.default_rng(12)
    E, S = sum(sizes), 3
    phi, e = [0.01, 0.003, 0.05], [0.1, 0.4, 0.2]
    probs = (0.025, 0.25, 0.975)
    K = len(probs)
    tot = rng.integers(0, 700, (E, S)).astype(np.int64)
    tot[[0, 5, 129, 130, 141], 1] = 0
    on = [(10, 0, 0), (20, 0, 2), (70, 1, 1), (140, 2, 0), (196, 0, 1)]      # (exon, sample, k): the count goes onto cut k, the next exon's below it
    for x, s, _ in on:
        tot[x:x + 2, s] = 500
    test = rng.binomial(tot, np.array(e)[None, :]).astype(np.int64)
    top = edlib.quantile_geometry()["max_total"]
    tot[[3, 64, 200], 2] = top + 7                                     # skipped exons inside the runs
    plan, qm = make_map(edlib, sizes, test, tot - test, phi, e, probs)
    ex = qm.exons()
    q, bl = ex[0], ex[1]                                               # (K, S, E)
    # ties: the test count of some exons is put on a cut, and one below it
    cut = np.vectorize(qc.cut_of, otypes=[np.int64])
    for x, s, k in on:
        c = int(cut(q[k, s, x]))
        assert 0 < c <= tot[x, s]
        test[x, s] = c
        assert cut(q[k, s, x + 1]) == c                              # (the same total: the same cut)
        test[x + 1, s] = c - 1
    qm.free()
    qm = plan.quantile_map(test.astype(np.int32), (tot - test).astype(np.int32), phi, e, probs)
    assert same_bits(qm.exons(), ex)                                   # the map depends on the totals alone
    rows = [(0, 17, 17), (0, 0, 0), (0, 0, 63), (0, 0, 64), (0, 0, 129), (1, 130, 130), (2, 131, 195), (2, 140, 150), (4, 196, 259), (4, 200, 200)]
    reg = qm.regions(rows + [(3, -1, -1)])
    assert reg["observed"].shape == (len(rows) + 1, S, K + 1) and reg["observed"].dtype == np.int32
    worst = 0.0
    for r, (c, lo, hi) in enumerate(rows):
        for s in range(S):
            valid = ~np.isnan(q[0, s, lo:hi + 1])
            assert reg["n_empty"][r, s] == int(np.sum(~valid)) == int(np.sum(tot[lo:hi + 1, s] > top))
            cuts = cut(q[:, s, lo:hi + 1])                              # (K, len)
            bins = np.sum(test[lo:hi + 1, s][None, :] >= cuts, axis=0)
            want = np.array([np.sum((bins == bb) & valid) for bb in range(K + 1)])
            assert np.array_equal(reg["observed"][r, s], want), (r, s)
            edges = np.concatenate([np.zeros((1, hi - lo + 1)), bl[:, s, lo:hi + 1], np.ones((1, hi - lo + 1))])
            for bb in range(K + 1):
                terms = np.where(valid, edges[bb + 1] - edges[bb], 0.0)
                assert bits(reg["expected"][r, s, bb]) == bits(qc.region_sum(terms)), (r, s, bb)
            nv = int(valid.sum())
            err = abs(math.fsum(reg["expected"][r, s]) - nv)
            worst = max(worst, err / max(nv, 1))
            assert err <= nv * 2.0 ** -52, (r, s, err)
            ev = reg["expected"][r, s]
            chi = float(np.sum(np.where(ev > 0, (reg["observed"][r, s] - ev) ** 2 / np.where(ev > 0, ev, 1.0), 0.0)))
            assert abs(reg["chi2"][r, s] - chi) <= 1e-12 * max(chi, 1.0)
    for x, s, k in on:                                                 # a count on a cut is in the upper bin, one below it in the lower
        r = qm.regions([(int(np.searchsorted(plan.chrom_off, x, "right")) - 1, x, x), (int(np.searchsorted(plan.chrom_off, x, "right")) - 1, x + 1, x + 1)])
        b_on = int(np.flatnonzero(reg_one(r, 0, s))[0])
        assert b_on >= k + 1 and b_on == int(np.sum(test[x, s] >= cut(q[:, s, x])))
        assert int(np.flatnonzero(reg_one(r, 1, s))[0]) <= k
    last = len(rows)                                                   # a region with no exon inside
    assert np.all(reg["observed"][last] == 0) and np.all(reg["expected"][last] == 0.0) and np.all(reg["n_empty"][last] == 0) and np.all(reg["chi2"][last] == 0.0)
    print("largest |sum of expected - exons| / exons: %.3g (2^-52 = %.3g)" % (worst, 2.0 ** -52))
    qm.free()
    plan.close()


def reg_one(r, row, s):
    v = r["observed"][row, s]
    assert v.sum() == 1
    return v


def test_calibration_of_a_well_specified_sample(edlib):
    """counts drawn from the fitted model fall into the bins as the model says: chi2 over the whole exome is small"""
    rng = np.random.default_rng(20261020)
    E, phi, e = 20000, 0.01, 0.25
    tot = rng.integers(200, 1200, E)
    a, b = qc.shapes(phi, e)
    test = rng.binomial(tot, rng.beta(a, b, E))
    probs = (0.025, 0.25, 0.5, 0.75, 0.975)
    ex, reg = edlib.normal_range([0, E], np.arange(E) * 1000 + 1, np.arange(E) * 1000 + 121, test.astype(np.int32)[:, None],
                                 (tot - test).astype(np.int32)[:, None], [phi], [e], rows=[(0, 0, E - 1)], probs=probs)
    obs, exp = reg["observed"][0, 0], reg["expected"][0, 0]
    print("observed", obs, "expected", np.round(exp, 1), "chi2 %.2f on %d bins" % (reg["chi2"][0, 0], obs.size))
    assert obs.sum() == E and abs(exp.sum() - E) <= E * 2.0 ** -52
    assert reg["chi2"][0, 0] < 33.0                    # chi-square, 5 degrees of freedom: 1e-5 lies above 30.9
    shifted = np.minimum(tot, (test * 1.1).astype(np.int64))           # 10 % more test reads: the same model no longer fits
    _, reg2 = edlib.normal_range([0, E], np.arange(E) * 1000 + 1, np.arange(E) * 1000 + 121, shifted.astype(np.int32)[:, None],
                                 (tot - shifted).astype(np.int32)[:, None], [phi], [e], rows=[(0, 0, E - 1)], probs=probs)
    assert reg2["chi2"][0, 0] > 10 * 33.0


# ---- 7. surfaces ----------------------------------------------------------------------------------------------------------------
def _exome_case():
    rng = np.random.default_rng(77)
    sizes = {"2": 40, "1": 70, "X": 30}
    chrom, start = [], []
    for c, m in sizes.items():
        chrom += [c] * m
        start += list(np.arange(m) * 4000 + 100)
    chrom, start = np.array(chrom, dtype=object), np.array(start)
    end = start + 200
    ref = rng.integers(150, 550, chrom.size).astype(np.float64)
    test = rng.binomial(ref.astype(np.int64) * 2, 0.25).astype(np.float64)
    k = np.flatnonzero(chrom == "1")[30:44]
    test[k] = np.round(test[k] * 0.5)          # a deletion on chromosome 1
    test[np.flatnonzero(chrom == "1")[50:53]] *= 2.0          # and three exons far above
    return chrom, start, end, test, ref


def _restated_plot_frame(x, sequence, xlim, count_threshold, probs):
    """R/plot_CNVs_method.R:33-63 in numpy, qbetabinom by the scipy restatement of R/tools.R:42-53"""
    anno = {k: np.asarray(v, dtype=object if k == "chromosome" else None) for k, v in x.annotations.items() if k != "name"}
    sel = np.flatnonzero((anno["chromosome"] == sequence) & (anno["start"] >= xlim[0]) & (anno["end"] <= xlim[1]) &
                         ((x.test + x.reference) * x.expected > count_threshold))
    if sel.size == 0:
        return None
    f = {"expected": x.expected[sel], "freq": x.test[sel] / (x.reference[sel] + x.test[sel]), "middle": 0.5 * (anno["start"][sel] + anno["end"][sel])}
    f["ratio"] = f["freq"] / f["expected"]
    f["test"], f["reference"] = x.test[sel], x.reference[sel]
    f["total_counts"] = f["test"] + f["reference"]
    f["phi"] = x.phi[sel]
    for name, p in (("my_min_norm", probs[0]), ("my_max_norm", probs[1])):
        f[name] = np.array([qc.scipy_qbetabinom_ab(p, n, *qc.shapes(ph, ex)) for n, ph, ex in zip(f["total_counts"], f["phi"], f["expected"])])
        f[name + "_prop"] = f[name] / f["total_counts"]
    return f


@pytest.mark.parametrize("per_exon_phi", [False, True])
def test_exomedepth_normal_range(edlib, per_exon_phi):
    chrom, start, end, test, ref = _exome_case()
    order, _, _, _ = edlib.chromosome_order(chrom, start, end)
    chrom, start, end, test, ref = chrom[order], start[order], end[order], test[order], ref[order]
    phi = np.linspace(0.001, 0.004, chrom.size) if per_exon_phi else 0.002
    x = edlib.ExomeDepth(test, ref, phi=phi, expected=0.33)
    with pytest.raises(ValueError, match="position of the exons"):
        x.normal_range("1", (0, 10 ** 7))
    x.CallCNVs(chrom, start, end, np.array(["e%d" % i for i in range(chrom.size)], dtype=object))
    calls = [dict(c) for c in x.CNV_calls]
    xlim, probs = (4000 * 5, 4000 * 60 + 300), (0.025, 0.975)
    got = x.normal_range("1", xlim)
    want = _restated_plot_frame(x, "1", xlim, 10, probs)
    assert x.CNV_calls == calls                                   # nothing of the object is changed
    assert list(got) == ["middle", "ratio", "test", "reference", "total_counts", "phi", "my_min_norm", "my_max_norm", "my_min_norm_prop",
                         "my_max_norm_prop", "outside"]
    assert want["middle"].size == 56 and (np.unique(got["phi"]).size > 1) == per_exon_phi
    for k in ("middle", "ratio", "test", "reference", "total_counts", "phi"):
        assert np.array_equal(got[k], want[k]), k
    worst = 0.0
    for name, p in (("my_min_norm", probs[0]), ("my_max_norm", probs[1])):
        for i in range(want["middle"].size):
            n, (a, b) = int(want["total_counts"][i]), qc.shapes(want["phi"][i], 0.33)
            frac, tol = qc.judge(float(got[name][i]), None, n, a, b, p)
            worst = max(worst, frac)
            assert frac <= 1.0
            # the scipy restatement is good to 2e-9 in probability (tests/test_quantile_host.py): the same value, next to it
            assert abs(float(qc.G(want[name][i], n, a, b)) - float(qc.G(got[name][i], n, a, b))) <= 2e-9 + tol
        assert same_bits(got[name], edlib.qbetabinom(p, want["total_counts"], want["phi"], 0.33))
        assert same_bits(got[name + "_prop"], got[name] / want["total_counts"])
    lo, hi = got["my_min_norm_prop"] / 0.33, got["my_max_norm_prop"] / 0.33
    assert np.array_equal(got["outside"], (got["ratio"] > hi).astype(np.int8) - (got["ratio"] < lo).astype(np.int8))
    inside_deletion = (got["middle"] > 4000 * 30) & (got["middle"] < 4000 * 44)
    assert np.sum(got["outside"][inside_deletion] == -1) >= 10 and np.sum(got["outside"] == 1) >= 3 and np.sum(got["outside"] == 0) >= 30
    print("largest fraction of the bar %.3g; outside: %d below, %d above of %d" % (worst, np.sum(got["outside"] == -1), np.sum(got["outside"] == 1), got["outside"].size))
    # the count threshold, other probabilities, an empty selection
    few = x.normal_range("1", xlim, count_threshold=150)
    assert 0 < few["middle"].size < got["middle"].size and np.all(few["total_counts"] * 0.33 > 150)
    wide = x.normal_range("1", xlim, probs=(0.001, 0.999))
    assert np.all(wide["my_min_norm"] < got["my_min_norm"]) and np.all(wide["my_max_norm"] > got["my_max_norm"])
    assert x.normal_range("7", xlim) is None and x.normal_range("1", (5, 50)) is None and x.normal_range("1", xlim, count_threshold=10 ** 6) is None
    assert _restated_plot_frame(x, "7", xlim, 10, probs) is None


def test_cohort_function(edlib):
    sizes, test, ref, phi, e, rows = _inv_case()
    chrom_off, start, end = design(sizes)
    cols = [0, 33, 5]
    ex, reg = edlib.normal_range(chrom_off, start, end, test[:, cols], ref[:, cols], phi[cols], e[cols], rows=rows)
    only = edlib.normal_range(chrom_off, start, end, test[:, cols], ref[:, cols], phi[cols], e[cols])
    plan, qm = make_map(edlib, sizes, test[:, [33]], ref[:, [33]], phi[[33]], e[[33]])
    own = qm.regions(rows)
    assert ex.shape == (2, 2, 3, sum(sizes)) and same_bits(only, ex) and same_bits(qm.exons()[:, :, 0], ex[:, :, 1])
    for k in ("observed", "expected", "n_empty", "chi2"):
        assert own[k][:, 0].tobytes() == np.ascontiguousarray(reg[k][:, 1]).tobytes(), k
    qm.free()
    plan.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(edlib):
    from exomedepth_amd import _lib
    lib = _lib.lib()
    sizes = [10, 0, 6]
    rng = np.random.default_rng(4)
    tot = rng.integers(0, 300, (16, 3)).astype(np.int32)
    plan, qm = make_map(edlib, sizes, np.zeros_like(tot), tot, [0.01, 0.02, 0.02], [0.1, 0.1, 0.2])

    def live():
        n, b = C.c_int64(), C.c_int64()
        lib.ed_live_allocations(C.byref(n), C.byref(b))
        return n.value

    live0 = live()
    z = np.zeros((16, 3), np.int32)
    for probs, what in (((), "1 .. 16 probabilities"), (tuple(np.arange(1, 18) / 20.0), "1 .. 16 probabilities"), ((0.1, np.nan), "not finite"),
                        ((0.1, np.inf), "not finite"), ((0.0, 0.5), r"outside \(0, 1\)"), ((0.5, 1.0), r"outside \(0, 1\)"),
                        ((-0.1,), r"outside \(0, 1\)"), ((0.5, 0.5), "strictly ascending"), ((0.975, 0.025), "strictly ascending")):
        with pytest.raises(edlib.EdError, match=what) as err:
            plan.quantile_map(z, z, [0.01] * 3, [0.1] * 3, probs)
        assert "status -1" in str(err.value)
    with pytest.raises(edlib.EdError, match="layout 2"):
        _raw_map(lib, plan, z, layout=2)
    with pytest.raises(edlib.EdError, match="n_samples is outside"):
        _raw_map(lib, plan, z, n_samples=2 ** 20 + 1)
    with pytest.raises(edlib.EdError, match="n_samples is outside"):
        _raw_map(lib, plan, z, n_samples=0)
    with pytest.raises(ValueError, match="counts must have shape"):           # a shape that is not the plan's, or the other layout's
        plan.quantile_map(z.T.copy(), z.T.copy(), [0.01] * 3, [0.1] * 3)
    with pytest.raises(ValueError, match="counts must have shape"):
        plan.quantile_map(z[:15], z[:15], [0.01] * 3, [0.1] * 3)
    with pytest.raises(ValueError, match="one value per sample"):
        plan.quantile_map(z, z, [0.01] * 3, [0.1] * 2)
    for row, what in (((0, 5, 4), "first > last"), ((3, 0, 0), "chromosome outside"), ((-1, 0, 0), "chromosome outside"),
                      ((0, 8, 11), "inside its chromosome"), ((2, 9, 12), "inside its chromosome"), ((1, 10, 10), "inside its chromosome"),
                      ((2, 10, 16), "inside its chromosome"), ((0, -2, 3), "inside its chromosome")):
        with pytest.raises(edlib.EdError, match=what) as err:
            qm.regions([(0, 0, 3), row])
        assert "status -1" in str(err.value)
    assert live() == live0                                   # a refused call allocated nothing: nothing was enqueued
    rows = np.zeros(1, dtype=edlib.api.CALL_DTYPE)
    o4, o8 = np.zeros(9, np.int32), np.zeros(9)
    args = dict(map=qm.handle, rows=rows.ctypes.data, obs=o4.ctypes.data, exp=o8.ctypes.data, empty=o4.ctypes.data)
    for null in ("map", "rows", "obs", "exp", "empty"):
        a = dict(args, **{null: None})
        assert lib.ed_quant_regions(a["map"], a["rows"], 1, a["obs"], a["exp"], a["empty"], None) == -1, null
    assert lib.ed_quant_regions(qm.handle, rows.ctypes.data, -1, o4.ctypes.data, o8.ctypes.data, o4.ctypes.data, None) == -1
    h = C.c_void_p()
    one, band = np.array([0.01]), np.array([0.025, 0.975])
    ok = [C.byref(h), plan.handle, z.ctypes.data, z.ctypes.data, 0, 0, one.ctypes.data, one.ctypes.data, band.ctypes.data, 2, 1, None]
    for i in (0, 1, 2, 3, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert lib.ed_plan_quantile_map(*bad) == -1, i
    assert not h.value
    assert lib.ed_quant_geometry(None) == -1 and lib.ed_quant_stats(None, None, None) == -1 and lib.ed_quant_copy_exons(None, None, None) == -1
    n = C.c_int64()
    assert lib.ed_quant_copy_table(qm.handle, 3, None, None, 0, C.byref(n)) == -1 and lib.ed_quant_copy_table(qm.handle, -1, None, None, 0, C.byref(n)) == -1
    assert lib.ed_qbetabinom_ab(None, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data) == -1
    assert lib.ed_qbetabinom_ab(one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, -1, one.ctypes.data) == -1
    assert live() == live0
    qm.free()
    qm.free()                                                # twice is harmless
    plan.close()
    assert live() < live0                                    # the map's buffers went with it


def _raw_map(lib, plan, z, layout=0, n_samples=3):
    """ed_plan_quantile_map with arguments the Python surface would not let through"""
    from exomedepth_amd._lib import check
    h = C.c_void_p()
    par, band = np.full(3, 0.05), np.array([0.025, 0.975])
    try:
        check(lib.ed_plan_quantile_map(C.byref(h), plan.handle, z.ctypes.data, z.ctypes.data, 0, layout, par.ctypes.data, par.ctypes.data,
                                       band.ctypes.data, 2, n_samples, None))
    finally:
        assert not h.value


# ---- 8. the shared map core -----------------------------------------------------------------------------------------------------
def test_power_and_quantile_maps_share_their_occupancy(edlib):
    """A PowerMap and a QuantileMap of the same counts stand on one occupancy (csrc/edtotals.inc: pw_occupy, TotalsMap): every sample's
    table lists the same totals, and the eight common counters agree but for the samples outside the model, which each map judges by
    its own shapes -- here both refuse the same one.  Input: tools/dump_total_maps.py's 131 exons x 5 samples, narrow and wide map."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("dump_total_maps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools",
                                                                                  "dump_total_maps.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = edlib.quantile_geometry()
    plan = edlib.Plan(*tool.design())
    common = ("n_samples", "n_exons", "n_jobs", "max_jobs", "n_skipped", "n_bad_samples", "largest_total", "map_words")
    for wide in (False, True):
        test, ref = tool.counts(g, wide)
        assert test.shape == (131, 5)
        pm, qm = plan.power_map(test, ref, tool.PHI, tool.EXPECTED), plan.quantile_map(test, ref, tool.PHI, tool.EXPECTED)
        ps, qs = pm.stats(), qm.stats()
        assert [ps[k] for k in common] == [qs[k] for k in common], (ps, qs)
        assert ps["n_skipped"] == 1 and ps["n_bad_samples"] == 1 and ps["largest_total"] == (g["max_total"] if wide else g["occupancy_cap"] - 1)
        for s in range(5):
            tp, tq = pm.table(s)["totals"], qm.table(s)["totals"]
            assert tp.dtype == tq.dtype == np.int32 and np.array_equal(tp, tq), s
            assert set(tool.edge_totals(g, wide)) <= set(tp.tolist())
        pm.free()
        qm.free()
    plan.close()
