"""The detection-power map on the GPU (csrc/edpower.inc) against the 40-digit checker (tests/power_checker.py), against the decoder's own
emissions, bit for bit against itself, at the edges of its occupancy map and of its region sums, and through the Python surface.

The walk's bar is the project's bar for the mass-function walk (rtol 2e-10) stated on the absolute terms:
|mean - exact| <= 2e-10 E|D| and |var - exact| <= 2e-10 E[D^2], because the mean is a cancellation at small mixtures.
Figures measured on an MI355X when this file was written (the tests print them with -s): DESIGN.md 4.22.
"""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import betaln, gammaln

import posterior_checker as post
import power_checker as pc

pytestmark = pytest.mark.gpu

PHIS = (1e-5, 0.003, 0.05, 0.2)
EXPECTED = (0.05, 0.11, 0.4)
MIXTURES = (1.0, 0.3)
VAL = ("mean_del", "var_del", "mean_dup", "var_dup")
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def design(sizes, step=1000, width=120):
    """chrom_off, start, end of chromosomes of the given sizes (exon i of a chromosome at i * step + 1)"""
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    start = np.concatenate([np.arange(m, dtype=np.int64) * step + 1 for m in sizes] + [np.zeros(0, np.int64)]).astype(np.int32)
    return chrom_off, start, (start + width).astype(np.int32)


def make_map(edlib, sizes, totals, phi, expected, mixture=1.0, layout=0, device=False):
    """totals (E, S): every total is put into the reference count (a value depends on the total alone)"""
    chrom_off, start, end = design(sizes)
    plan = edlib.Plan(chrom_off, start, end)
    ref = np.ascontiguousarray(totals, dtype=np.int32)
    rng = np.random.default_rng(3)
    test = np.minimum(rng.integers(0, 7, ref.shape).astype(np.int32), ref)      # part of the total on either side
    ref = ref - test
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    if device:
        test, ref = edlib.DeviceArray(test), edlib.DeviceArray(ref)
    pm = plan.power_map(test, ref, phi, expected, mixture, layout=layout)
    if device:
        test.free()
        ref.free()
    return plan, pm


def table_of(pm, s):
    t = pm.table(s)
    return t["totals"], np.stack([t[k] for k in VAL])


def edge_totals(edlib):
    W = edlib.power_geometry()["walk_tile"]
    return [0, 1, 3, 4, 5] + [t + d for t in (W, 2 * W, 4 * W) for d in (-1, 0, 1)]


def _edge_map(edlib):
    if "edge" not in _CACHE:
        totals = edge_totals(edlib)
        par = [(p, e, m) for p in PHIS for e in EXPECTED for m in MIXTURES]
        S = len(par)
        tot = np.repeat(np.array(totals, dtype=np.int32)[:, None], S, axis=1)
        plan, pm = make_map(edlib, [len(totals)], tot, [q[0] for q in par], [q[1] for q in par], np.array([q[2] for q in par]))
        tabs = [table_of(pm, s) for s in range(S)]
        st = pm.stats()
        pm.free()
        plan.close()
        _CACHE["edge"] = (totals, par, tabs, st)
    return _CACHE["edge"]


# ---- 1. accuracy at the walk's edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", PHIS)
def test_walk_edges_against_the_checker(edlib, phi):
    totals, par, tabs, st = _edge_map(edlib)
    assert st["n_bad_samples"] == 0 and st["n_skipped"] == 0 and st["n_jobs"] == len(totals) * len(par)
    worst = 0.0
    for s, (p, e, m) in enumerate(par):
        if p != phi:
            continue
        tn, tv = tabs[s]
        assert list(tn) == sorted(totals)
        for j, n in enumerate(tn):
            want = pc.moments(int(n), p, e, m)
            for c, T in ((0, "del"), (2, "dup")):
                bm, bv = pc.RTOL * want["abs_" + T], pc.RTOL * want["sq_" + T]
                em, ev = abs(tv[c, j] - want["mean_" + T]), abs(tv[c + 1, j] - want["var_" + T])
                if n == 0:
                    assert tv[c, j] == 0.0 and tv[c + 1, j] == 0.0
                    continue
                worst = max(worst, em / bm, ev / bv)
                assert em <= bm, (p, e, m, n, T, tv[c, j], want["mean_" + T], em / bm)
                assert ev <= bv, (p, e, m, n, T, tv[c + 1, j], want["var_" + T], ev / bv)
                assert tv[c, j] >= -bm and tv[c + 1, j] >= 0.0
    print("phi = %g: largest fraction of the bar %.3g" % (phi, worst))


# ---- 2. it is the decoder's model -------------------------------------------------------------------------------------------
def test_expected_evidence_matches_the_strict_emissions(edlib):
    E, phi, e = 20000, 0.01, 0.1
    rng = np.random.default_rng(20261020)
    total = rng.integers(300, 1501, E).astype(np.int32)
    plan, pm = make_map(edlib, [E], total[:, None], [phi], [e])
    ex = pm.exons()[:, 0, :]
    pm.free()
    plan.close()
    a1, a2 = pc.shape_params(phi, e, 1.0)
    for T, col, c in (("del", 0, 0), ("dup", 2, 2)):
        obs = rng.binomial(total, rng.beta(a1[col], a2[col], E)).astype(np.int32)
        ll = edlib.get_loglike_matrix(phi, e, total, obs)
        got = float(np.sum(ll[:, col] - ll[:, 1])) * math.log10(math.e)
        mean, sd = float(np.sum(ex[c])), math.sqrt(float(np.sum(ex[c + 1])))
        z = (got - mean) / sd
        print("%s: sum BF %.3f, expected %.3f, sd %.3f, z = %.2f" % (T, got, mean, sd, z))
        assert abs(got - mean) <= 5.0 * sd, (T, got, mean, sd)
        # the band tells models apart: the expectation under the constant-phi alternative of get.power.betabinom lies outside it
        f = 0.5 if T == "del" else 1.5
        pa = (e * f) / (e * f + 1 - e)
        aa, ab, a, b = pa * (1 - phi) / phi, (1 - pa) * (1 - phi) / phi, e * (1 - phi) / phi, (1 - e) * (1 - phi) / phi
        other = 0.0
        for n in np.unique(total):
            n0 = float(n)
            x = np.arange(n0 + 1)
            la, l0 = betaln(aa + x, ab + n0 - x) - betaln(aa, ab), betaln(a + x, b + n0 - x) - betaln(a, b)
            P = np.exp(gammaln(n0 + 1) - gammaln(x + 1) - gammaln(n0 - x + 1) + la)
            other += float(np.sum(P * (la - l0))) * math.log10(math.e) * int(np.sum(total == n))
        print("    constant-phi alternative: %.3f, %.1f sd away" % (other, (other - mean) / sd))
        assert abs(other - mean) > 5.0 * sd


# ---- 3. identical hypotheses ------------------------------------------------------------------------------------------------
def test_identical_hypotheses(edlib):
    totals = np.arange(0, 301, dtype=np.int32)
    par = [(p, e) for p in (0.003, 0.05) for e in (0.125, 0.25, 0.5)]
    S = len(par)
    plan, pm = make_map(edlib, [totals.size], np.repeat(totals[:, None], S, axis=1), [q[0] for q in par], [q[1] for q in par], 0.0)
    ex = pm.exons()
    pm.free()
    plan.close()
    assert np.all(np.isfinite(ex))
    print("largest |mean| %.3g, largest var %.3g" % (np.abs(ex[[0, 2]]).max(), ex[[1, 3]].max()))
    assert np.abs(ex[[0, 2]]).max() <= 1e-12 and np.abs(ex[[1, 3]]).max() <= 1e-12


# ---- 4. bit invariance ------------------------------------------------------------------------------------------------------
def _inv_case():
    rng = np.random.default_rng(41)
    sizes = [150, 0, 333, 70]
    E = sum(sizes)
    tot = rng.integers(0, 900, (E, 70)).astype(np.int32)
    tot[rng.choice(E, 9, replace=False), :] = 0
    phi, e, mix = rng.uniform(0.002, 0.05, 70), rng.uniform(0.08, 0.45, 70), rng.uniform(0.2, 1.0, 70)
    rows = [(0, 0, 149), (0, 7, 7), (2, 150, 482), (2, 200, 290), (3, 483, 552), (3, 500, 552), (0, 60, 130)]
    return sizes, tot, phi, e, mix, rows


def test_bit_invariance(edlib):
    sizes, tot, phi, e, mix, rows = _inv_case()
    the = 33                                          # the sample that is followed through the settings
    results = []
    for cols, layout, device in (([the], 0, False), ([the], 1, True), ([the, 1, 2, 3, 4], 0, True), ([the, 1, 2, 3, 4], 1, False),
                                 (list(range(69)) + [the], 0, False), (list(range(69)) + [the], 1, True)):
        at = cols.index(the)
        plan, pm = make_map(edlib, sizes, tot[:, cols], phi[cols], e[cols], mix[cols], layout=layout, device=device)
        order = list(range(len(rows))) if layout == 0 else [4, 2, 0, 6, 2, 1, 3, 5, 2]        # permuted and duplicated
        reg = pm.regions([rows[i] for i in order])[:, at]
        first = {}
        for k, i in enumerate(order):
            if i in first:
                assert reg[k].tobytes() == reg[first[i]].tobytes()
            first.setdefault(i, k)
        results.append((table_of(pm, at), pm.exons()[:, at, :], np.stack([reg[first[i]] for i in range(len(rows))])))
        pm.free()
        plan.close()
    (tn0, tv0), ex0, rg0 = results[0]
    assert tn0.size > 100 and np.all(np.isfinite(ex0))
    for (tn, tv), ex, rg in results[1:]:
        assert np.array_equal(tn, tn0) and same_bits(tv, tv0) and same_bits(ex, ex0)
        assert rg.tobytes() == rg0.tobytes()
    # a scalar mixture is the per-sample one
    plan, pm = make_map(edlib, sizes, tot[:, [the]], phi[[the]], e[[the]], float(mix[the]))
    assert same_bits(pm.exons()[:, 0, :], ex0)
    pm.free()
    plan.close()


# ---- 5. occupancy edges -----------------------------------------------------------------------------------------------------
def test_occupancy_edges(edlib):
    g = edlib.power_geometry()
    cap, top, RT = g["occupancy_cap"], g["max_total"], g["region_tile"]
    assert top >= 2 ** 20 and cap < top
    phi, e = [0.05], [0.1]
    # one job; every exon a total of its own
    plan, pm = make_map(edlib, [40], np.full((40, 1), 77, np.int32), phi, e)
    st, ex = pm.stats(), pm.exons()
    assert st["n_jobs"] == 1 and st["max_jobs"] == 1 and st["largest_total"] == 77 and st["map_words"] == cap // 32
    assert np.all(bits(ex) == bits(ex)[:, :, :1])
    one = ex[:, 0, 0]
    pm.free(); plan.close()
    distinct = np.arange(5, 5 + 300, dtype=np.int32)[::-1].copy()
    plan, pm = make_map(edlib, [300], distinct[:, None], phi, e)
    st, ex = pm.stats(), pm.exons()
    assert st["n_jobs"] == 300 and st["max_jobs"] == 300
    tn, tv = table_of(pm, 0)
    assert np.array_equal(tn, np.sort(distinct)) and same_bits(ex[:, 0, :], tv[:, ::-1])
    assert same_bits(ex[:, 0, list(distinct).index(77)], one)
    pm.free(); plan.close()
    # the occupancy cap: the narrow map holds cap - 1, the wide one takes over at cap
    plan, pm = make_map(edlib, [3], np.array([[cap - 1], [77], [0]], np.int32), phi, e)
    assert pm.stats()["map_words"] == cap // 32
    below = pm.exons()[:, 0, :]
    pm.free(); plan.close()
    plan, pm = make_map(edlib, [5], np.array([[cap - 1], [cap], [77], [cap + 1], [0]], np.int32), phi, e)
    st = pm.stats()
    assert st["map_words"] == top // 32 + 1 and st["n_jobs"] == 5 and st["largest_total"] == cap + 1
    wide = pm.exons()[:, 0, :]
    assert np.array_equal(table_of(pm, 0)[0], [0, 77, cap - 1, cap, cap + 1])
    pm.free(); plan.close()
    assert same_bits(wide[:, [0, 2, 4]], below) and same_bits(wide[:, 2], one)
    for col, n in ((0, cap - 1), (1, cap), (3, cap + 1)):
        want = pc.scipy_moments(n, phi[0], e[0])
        assert abs(wide[0, col] - want["mean_del"]) <= 1e-9 * want["mean_del"] and abs(wide[2, col] - want["mean_dup"]) <= 1e-9 * want["mean_dup"]
        assert abs(wide[1, col] - want["var_del"]) <= 1e-8 * want["var_del"] and abs(wide[3, col] - want["var_dup"]) <= 1e-8 * want["var_dup"]
    # one total above the maximum: NaN on its exon only
    tot = np.array([[12], [top + 1], [77], [top], [0]], np.int64)
    chrom_off, start, end = design([5])
    plan = edlib.Plan(chrom_off, start, end)
    ref = tot.astype(np.int32)
    pm = plan.power_map(np.zeros_like(ref), ref, phi, e)
    st, over = pm.stats(), pm.exons()[:, 0, :]
    assert st["n_skipped"] == 1 and st["n_jobs"] == 4 and st["largest_total"] == top
    reg = pm.regions([(0, 0, 4), (0, 2, 4)])[:, 0]
    assert np.isnan(reg["mean_del"][0]) and np.isnan(reg["power_dup"][0]) and np.isfinite(reg["mean_del"][1]) and reg["n_empty"][1] == 1
    pm.free()
    ref[1, 0] = 12
    pm = plan.power_map(np.zeros_like(ref), ref, phi, e)
    clean = pm.exons()[:, 0, :]
    assert pm.stats()["n_skipped"] == 0
    pm.free(); plan.close()
    assert np.all(np.isnan(over[:, 1])) and same_bits(over[:, [0, 2, 3, 4]], clean[:, [0, 2, 3, 4]]) and same_bits(clean[:, 2], one)
    assert np.all(over[:, 4] == 0.0) and np.all(np.isfinite(clean))
    # E = 1; an empty chromosome between two others; E around a multiple of the region tile
    plan, pm = make_map(edlib, [1], np.array([[77]], np.int32), phi, e)
    assert same_bits(pm.exons()[:, 0, 0], one) and same_bits(np.array([pm.regions([(0, 0, 0)])[0, 0][k] for k in VAL]), one)
    pm.free(); plan.close()
    rng = np.random.default_rng(8)
    for m in (2 * RT - 1, 2 * RT, 2 * RT + 1):
        tot = rng.integers(1, 400, (m + 3, 2)).astype(np.int32)
        plan, pm = make_map(edlib, [3, 0, m], tot, [0.05, 0.01], [0.1, 0.3])
        ex = pm.exons()
        reg = pm.regions([(2, 3, m + 2), (0, 0, 2)])
        with pytest.raises(edlib.EdError, match="inside its chromosome"):
            pm.regions([(1, 3, 3)])
        for s in range(2):
            for c, k in enumerate(VAL):
                assert bits(reg[k][0, s]) == bits(pc.region_sum(ex[c, s, 3:]))
                assert bits(reg[k][1, s]) == bits(pc.region_sum(ex[c, s, :3]))
        assert list(reg["n_exons"][:, 0]) == [m, 3]
        pm.free(); plan.close()


# ---- 6. regions -------------------------------------------------------------------------------------------------------------
def test_regions(edlib):
    sizes = [513, 1, 90]
    rng = np.random.default_rng(12)
    E, S = sum(sizes), 3
    tot = rng.integers(0, 700, (E, S)).astype(np.int32)
    tot[[0, 5, 512, 513, 600], 1] = 0
    chrom_off, start, end = design(sizes, step=7919)
    start = (start + rng.integers(0, 3000, E)).astype(np.int32)
    end = (start + 150).astype(np.int32)
    plan = edlib.Plan(chrom_off, start, end, 1e-4, 50000.0)
    pm = plan.power_map(np.zeros_like(tot), tot, [0.01, 0.003, 0.05], [0.1, 0.4, 0.2], np.array([1.0, 0.5, 1.0]))
    ex = pm.exons()
    rows = [(0, 17, 17), (0, 0, 0), (0, 512, 512), (0, 0, 512), (1, 513, 513), (2, 514, 603), (2, 520, 585), (0, 3, 130)]
    reg = pm.regions(rows)
    trs = post.transitions(chrom_off, start, end, 1e-4, 50000.0)
    for r, (c, a, b) in enumerate(rows):
        lo = int(chrom_off[c])
        want = pc.price(trs[c], a - lo, b - lo)
        assert abs(reg["price"][r, 0] - want) <= 1e-12 * abs(want), (r, reg["price"][r, 0], want)
        assert np.all(bits(reg["price"][r]) == bits(reg["price"][r, 0])) and np.all(reg["threshold"][r] == reg["price"][r])
        for s in range(S):
            assert reg["n_exons"][r, s] == b - a + 1 and reg["n_empty"][r, s] == int(np.sum(tot[a:b + 1, s] == 0))
            for ci, k in enumerate(VAL):
                v = ex[ci, s, a:b + 1]
                assert bits(reg[k][r, s]) == bits(pc.region_sum(v)), (r, s, k)
                assert abs(reg[k][r, s] - math.fsum(v)) <= (b - a + 1) * 2.0 ** -52 * math.fsum(v)
            for T in ("del", "dup"):
                m, v, p = reg["mean_" + T][r, s], reg["var_" + T][r, s], reg["power_" + T][r, s]
                assert p == edlib.power_from_moments(m, v, reg["price"][r, s]) and 0.0 <= p <= 1.0
    assert reg["price"][3, 0] > reg["price"][0, 0] > 0            # a longer segment costs more
    assert np.all(reg["mean_del"][3] > reg["mean_del"][7]) and np.all(reg["power_del"][3, :2] > 0.99)
    # a threshold of one's own, and a region without exons
    own = pm.regions([(0, 3, 130), (0, -1, -1)], threshold=[5.0, 5.0])
    assert np.all(own["threshold"] == 5.0) and np.all(own["n_exons"][1] == 0) and np.all(np.isnan(own["price"][1]))
    assert np.all(own["mean_del"][1] == 0.0) and np.all(own["power_del"][1] == 0.0) and same_bits(own["mean_del"][0], reg["mean_del"][7])
    pm.free()
    plan.close()


def test_a_call_table_is_a_region_list(edlib):
    sizes = [200, 120]
    E = sum(sizes)
    chrom_off, start, end = design(sizes)
    rng = np.random.default_rng(2)
    ref = rng.integers(380, 420, (E, 2)).astype(np.int32)
    test = ref.copy()
    test[40:52, 0] //= 2                       # a deletion in sample 0
    test[250:270, 1] = test[250:270, 1] * 3 // 2        # a duplication in sample 1
    plan = edlib.Plan(chrom_off, start, end)
    b = edlib.Batch(plan, 2)
    b.run(test, ref, np.array([0.001, 0.001]), np.array([0.5, 0.5]))
    calls = b.calls()
    b.close()
    assert calls.size >= 2
    pm = plan.power_map(test, ref, [0.001, 0.001], [0.5, 0.5])
    reg = pm.regions(calls)
    assert reg.shape == (calls.size, 2)
    assert np.array_equal(reg["n_exons"][:, 0], calls["nexons"]) and np.array_equal(reg["first_exon"][:, 0], calls["start_exon"])
    for r, c in enumerate(calls):
        k = "power_del" if c["type"] == 1 else "power_dup"
        assert reg[k][r, c["sample"]] > 0.99      # what was called could be seen
    pm.free()
    plan.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(edlib):
    from exomedepth_amd import _lib
    lib = _lib.lib()
    sizes = [10, 0, 6]
    rng = np.random.default_rng(4)
    tot = rng.integers(0, 300, (16, 3)).astype(np.int32)
    plan, pm = make_map(edlib, sizes, tot, [0.01, 0.9, 0.02], [0.1, 0.1, 0.2])
    st = pm.stats()
    assert st["n_bad_samples"] == 1
    ex = pm.exons()
    assert np.all(np.isnan(ex[:, 1, :])) and np.all(np.isfinite(ex[:, [0, 2], :]))
    t1 = pm.table(1)
    assert t1["totals"].size == np.unique(tot[:, 1]).size and np.all(np.isnan(t1["mean_del"]))
    reg = pm.regions([(0, 0, 9)])
    assert np.isnan(reg["mean_dup"][0, 1]) and np.isnan(reg["power_del"][0, 1]) and np.isfinite(reg["mean_dup"][0, 0])
    plan2, pm2 = make_map(edlib, sizes, tot[:, [0, 2]], [0.01, 0.02], [0.1, 0.2])
    assert pm2.stats()["n_bad_samples"] == 0 and same_bits(pm2.exons(), ex[:, [0, 2], :])        # the batch-mates do not notice
    pm2.free(); plan2.close()
    live0 = (C.c_int64(), C.c_int64())
    lib.ed_live_allocations(C.byref(live0[0]), C.byref(live0[1]))
    for row, what in (((0, 5, 4), "first > last"), ((3, 0, 0), "chromosome outside"), ((-1, 0, 0), "chromosome outside"),
                      ((0, 8, 11), "inside its chromosome"), ((2, 9, 12), "inside its chromosome"), ((1, 10, 10), "inside its chromosome"),
                      ((2, 10, 16), "inside its chromosome"), ((0, -2, 3), "inside its chromosome")):
        with pytest.raises(edlib.EdError, match=what) as err:
            pm.regions([(0, 0, 3), row])
        assert "status -1" in str(err.value)
    live1 = (C.c_int64(), C.c_int64())
    lib.ed_live_allocations(C.byref(live1[0]), C.byref(live1[1]))
    assert live0[0].value == live1[0].value                  # a refused call allocated nothing: nothing was enqueued
    rows = np.zeros(1, dtype=edlib.api.CALL_DTYPE)
    out8, out4 = np.zeros(12), np.zeros(3, np.int32)
    args = dict(map=pm.handle, rows=rows.ctypes.data, n=1, sums=out8.ctypes.data, empty=out4.ctypes.data, price=out8.ctypes.data, nex=out4.ctypes.data)
    for null in ("map", "rows", "sums", "empty", "price", "nex"):
        a = dict(args, **{null: None})
        assert lib.ed_power_regions(a["map"], a["rows"], a["n"], a["sums"], a["empty"], a["price"], a["nex"], None) == -1, null
    assert lib.ed_power_regions(pm.handle, rows.ctypes.data, -1, out8.ctypes.data, out4.ctypes.data, out8.ctypes.data, out4.ctypes.data, None) == -1
    h = C.c_void_p()
    z = np.zeros(16, np.int32)
    one = np.array([0.01])
    assert lib.ed_plan_power_map(C.byref(h), None, z.ctypes.data, z.ctypes.data, 0, 0, 1, one.ctypes.data, one.ctypes.data, None, 1.0, None) == -1
    assert lib.ed_plan_power_map(C.byref(h), plan.handle, None, z.ctypes.data, 0, 0, 1, one.ctypes.data, one.ctypes.data, None, 1.0, None) == -1
    assert lib.ed_plan_power_map(C.byref(h), plan.handle, z.ctypes.data, z.ctypes.data, 0, 2, 1, one.ctypes.data, one.ctypes.data, None, 1.0, None) == -1
    assert lib.ed_plan_power_map(C.byref(h), plan.handle, z.ctypes.data, z.ctypes.data, 0, 0, 0, one.ctypes.data, one.ctypes.data, None, 1.0, None) == -1
    assert lib.ed_plan_power_map(C.byref(h), plan.handle, z.ctypes.data, z.ctypes.data, 0, 0, 1, None, one.ctypes.data, None, 1.0, None) == -1
    assert not h.value
    assert lib.ed_power_geometry(None) == -1 and lib.ed_power_stats(None, None, None) == -1
    pm.free()
    pm.free()                                                # twice is harmless
    plan.close()
    lib.ed_live_allocations(C.byref(live1[0]), C.byref(live1[1]))
    assert live1[0].value < live0[0].value                   # the map's buffers went with it


# ---- 8. surface -------------------------------------------------------------------------------------------------------------
def _exome_case():
    rng = np.random.default_rng(77)
    sizes = {"2": 90, "1": 140, "X": 60}
    chrom, start = [], []
    for c, m in sizes.items():
        chrom += [c] * m
        start += list(np.arange(m) * 4000 + 100)
    chrom, start = np.array(chrom, dtype=object), np.array(start)
    end = start + 200
    ref = rng.integers(450, 550, chrom.size).astype(np.float64)
    test = rng.binomial(ref.astype(np.int64) * 2, 0.25).astype(np.float64)
    k = np.flatnonzero(chrom == "1")[30:44]
    test[k] = np.round(test[k] * 0.5)          # a deletion on chromosome 1
    perm = rng.permutation(chrom.size)
    return chrom, start, end, test, ref, perm


def test_exomedepth_surface(edlib):
    chrom, start, end, test, ref, perm = _exome_case()
    regions = [("1", 100, 4000 * 20), ("1", 4000 * 30, 4000 * 44), ("X", 0, 10 ** 7), ("2", 150, 250), ("5", 0, 100)]
    order, _, _, _ = edlib.chromosome_order(chrom, start, end)
    srt = edlib.ExomeDepth(test[order], ref[order], phi=0.002, expected=0.33)
    a = srt.detection_power(chrom[order], start[order], end[order], regions)
    uns = edlib.ExomeDepth(test[perm], ref[perm], phi=0.002, expected=0.33)
    b = uns.detection_power(chrom[perm], start[perm], end[perm], regions)
    assert a.dtype == edlib.POWER_DTYPE and a.shape == (len(regions),) and a.tobytes() == b.tobytes()
    assert list(a["n_exons"]) == [20, 14, 60, 0, 0] and np.isnan(a["price"][3]) and a["power_del"][2] > 0.99
    assert np.array_equal(uns.test, test[perm])                                   # nothing of the object is changed
    with pytest.raises(ValueError, match="CallCNVs first"):
        srt.detection_power(chrom[order], start[order], end[order])
    name = np.array(["e%d" % i for i in range(chrom.size)], dtype=object)
    srt.CallCNVs(chrom[order], start[order], end[order], name[order])
    before = [dict(c) for c in srt.CNV_calls]
    assert len(before) >= 1
    own = srt.detection_power(chrom[order], start[order], end[order])
    assert own.shape == (len(before),) and [int(x) for x in own["first_exon"]] == [c["start.p"] - 1 for c in before]
    assert [int(x) for x in own["n_exons"]] == [c["end.p"] - c["start.p"] + 1 for c in before]
    again = edlib.ExomeDepth(test[order], ref[order], phi=0.002, expected=0.33).CallCNVs(chrom[order], start[order], end[order], name[order])
    assert srt.CNV_calls == before == again.CNV_calls                             # CallCNVs' output is what it was
    rng = np.random.default_rng(9)                   # depths that fill every level of the binning, a dispersion that grows with the depth
    depth = rng.integers(30, 3000, chrom.size)
    phi_true = np.where(depth < 1200, 0.002, 0.03)
    share = rng.beta(0.33 * (1 - phi_true) / phi_true, 0.67 * (1 - phi_true) / phi_true)
    few = rng.binomial(depth, share)
    binned = edlib.ExomeDepth(few.astype(np.float64), (depth - few).astype(np.float64), phi_bins=3)
    assert not np.all(binned.phi == binned.phi[0])
    with pytest.raises(NotImplementedError, match="per-exon"):
        binned.detection_power(chrom[order], start[order], end[order], regions)
    given = edlib.ExomeDepth(test[order], ref[order], phi=np.linspace(0.001, 0.003, chrom.size), expected=0.33)      # a per-exon phi handed in
    with pytest.raises(NotImplementedError, match="per-exon"):
        given.detection_power(chrom[order], start[order], end[order], regions)


def test_cohort_function(edlib):
    sizes, tot, phi, e, mix, rows = _inv_case()
    chrom_off, start, end = design(sizes)
    cols = [0, 33, 5]
    reg, ex = edlib.detection_power(chrom_off, start, end, np.zeros_like(tot[:, cols]), tot[:, cols], phi[cols], e[cols], rows, mixture=mix[cols],
                                    exons=True)
    plan, pm = make_map(edlib, sizes, tot[:, [33]], phi[[33]], e[[33]], mix[[33]])
    assert same_bits(pm.exons()[:, 0], ex[:, 1]) and pm.regions(rows)[:, 0].tobytes() == reg[:, 1].tobytes()
    pm.free()
    plan.close()
