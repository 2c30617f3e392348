"""Draws from the fitted model on the GPU (csrc/edsim.inc): the uniforms bit for bit against the checker's Philox, every
draw judged in probability space against the 40-digit checker with the bar of the walk's own operations, the cohort draw against the
element-wise draw bit for bit at the chunk edges, its invariance under batch width / layout / sample0 / where the counts live, the null
call table against the pipeline fed by hand, planted cells, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_checker as qc  # noqa: E402
import simulate_checker as sc  # noqa: E402

pytestmark = pytest.mark.gpu

TOTALS = (0, 1, 2, 3, 5, 63, 64, 255, 256, 257, 511, 512, 513, 1025, 4099)
PHIS = (1e-5, 0.003, 0.05, 0.2)
EXPECTED = (0.05, 0.11, 0.4)


def _host(d):
    return d.to_host().copy()


def test_uniforms_are_the_checkers_bit_for_bit(edlib):
    rng = np.random.default_rng(1)
    n = 4096
    exon = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    exon[:4] = (0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
    sample = rng.integers(0, 2 ** 20, size=n, dtype=np.uint64)
    rep = rng.integers(0, 100, size=n, dtype=np.uint64)
    for seed, stream in ((0, 0), (12345, 1), (2 ** 63 + 2 ** 32 + 5, 0)):
        got = edlib.runif53(seed, exon, sample, rep, stream)
        want = sc.u53_many(seed, exon, sample, rep, stream)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
        assert got.min() >= 2.0 ** -53 and got.max() <= 1.0 - 2.0 ** -53
    # recycling, and the known answer of the all-zero counter: k = (0x6627e8d5 >> 12) 2^32 + 0xe169c58d
    got = edlib.runif53(0, [0, 0, 0], 0, 0)
    assert got.shape == (3,) and np.all(got == sc.u53_of(((0x6627e8d5 >> 12) << 32) | 0xe169c58d))
    assert edlib.runif53(0, np.zeros(0, np.int64), 0, 0).size == 0


@pytest.mark.parametrize("phi", PHIS)
def test_draws_judged_in_probability_space(edlib, phi):
    """Every total x expected of the grid at this phi: eight generated uniforms and the planted ones through rbetabinom_ab_u.  A device x
    for u is right if and only if C_chk(x - 1) <= u + bar and (C_chk(x) >= u - bar or x = n), bar = quantile_checker.bar(n, x, span):
    none excused.  Prints the largest deviation as a share of the bar."""
    cases = []
    for e in EXPECTED:
        a, b = sc.shapes(phi, e)
        for n in TOTALS:
            us = [("generated", sc.u53(2024, k, n, int(e * 100)), None) for k in range(8)] + sc.planted_uniforms(n, a, b)
            cases += [(name, n, a, b, u) for name, u, _ in us]
    u = np.array([c[4] for c in cases])
    got = edlib.rbetabinom_ab_u(u, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    assert got.dtype == np.int32 and got.shape == (len(cases),)
    worst, n_moved, by_name = 0.0, 0, {}
    for (name, n, a, b, uu), x in zip(cases, got.tolist()):
        assert 0 <= x <= n, (name, n, phi, uu, x)
        used, tol = sc.judge(x, n, a, b, uu)
        assert used <= 1.0, (name, n, phi, uu, x, sc.draw(n, a, b, uu), used, tol)
        worst = max(worst, used)
        n_moved += x != sc.draw(n, a, b, uu)
        by_name[name] = by_name.get(name, 0) + 1
        if name == "smallest":
            assert x == sc.draw(n, a, b, uu) or used <= 1.0
        if name == "largest" and x != n:                        # 1 - 2^-53 reads n, or a crossing within the bar
            assert used <= 1.0
    # the planted ones well inside a value name that value exactly, two uniforms in one value the same one
    k = 0
    while k < len(cases):
        name = cases[k][0]
        if name in ("two in one value", "adjacent values of one lane", "adjacent values of two lanes"):
            (_, n, a, b, u0), (_, _, _, _, u1) = cases[k], cases[k + 1]
            x0, x1 = int(got[k]), int(got[k + 1])
            assert (x0, x1) == (sc.draw(n, a, b, u0), sc.draw(n, a, b, u1)), (name, n, phi)
            assert x1 - x0 == (0 if name == "two in one value" else 1)
            if name == "adjacent values of one lane":
                assert x0 // 4 == x1 // 4
            if name == "adjacent values of two lanes":
                assert x0 // 4 + 1 == x1 // 4
            k += 2
        else:
            k += 1
    assert by_name["generated"] == 8 * len(TOTALS) * len(EXPECTED) and by_name["smallest"] == len(TOTALS) * len(EXPECTED)
    print("phi = %g: %d draws, largest deviation %.3g of the bar, %d beside the checker's own value (all within the bar of a step)"
          % (phi, len(cases), worst, n_moved))


def test_element_wise_validation_and_surfaces(edlib):
    a, b = sc.shapes(0.05, 0.11)
    mx = edlib.sim_geometry()["max_total"]
    u = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -0.1, 1.0, float("nan"), 0.5, 0.0]
    size = [10, 10.5, -1, mx + 1, 10, 10, 10, 10, 10, mx, 10]
    sa = [a, a, a, a, -1.0, float("inf"), a, a, a, a, a]
    got = edlib.rbetabinom_ab_u(u, size, sa, b)
    assert got[:9].tolist() == [sc.draw(10, a, b, 0.5), -1, -1, -1, -1, -1, -1, -1, -1]
    assert 0 <= got[9] <= mx and got[10] == 0
    assert edlib.rbetabinom_ab_u([], 5, a, b).size == 0
    # rbetabinom_ab: element i is the draw at the counter (index[i] or i, 0, replicate, 0); rbetabinom forms the shapes as qbetabinom does
    size = np.array([5, 63, 257, 600, 0, 4099])
    x = edlib.rbetabinom_ab(size, a, b, seed=99, replicate=3)
    assert x.tolist() == edlib.rbetabinom_ab_u(edlib.runif53(99, np.arange(6), 0, 3, 0), size, a, b).tolist()
    idx = np.array([7, 2 ** 31 + 1, 0, 5, 5, 9], dtype=np.uint64)
    y = edlib.rbetabinom_ab(size, a, b, seed=99, index=idx, replicate=3)
    assert y.tolist() == edlib.rbetabinom_ab_u(edlib.runif53(99, idx, 0, 3, 0), size, a, b).tolist()
    assert edlib.rbetabinom(size, 0.05, 0.11, seed=99, replicate=3).tolist() == x.tolist()
    assert edlib.rbetabinom(size[2], 0.05, 0.11, seed=99, index=2, replicate=3).tolist() == [x[2]]       # alone = in company
    assert edlib.rbetabinom(size, 0.05, 0.11, seed=98, replicate=3).tolist() != x.tolist()


# ---- the cohort draw ---------------------------------------------------------------------------------------------------------
GROUPS = (1, 63, 64, 65, 129, 300)             # exons of sample 0 sharing one total: the chunk edges
GROUP_TOTALS = (37, 100, 255, 256, 1025, 600)  # the 300 share n = 600: at phi = 0.2 their uniforms cross in tiles 0, 1 and 2
SEED3 = 4242


def _cohort3(max_total):
    E = sum(GROUPS) + 2
    S = 3
    rng = np.random.default_rng(8)
    total = np.zeros((E, S), dtype=np.int64)
    order = rng.permutation(sum(GROUPS))                          # the groups' exons interleaved
    total[order, 0] = np.repeat(GROUP_TOTALS, GROUPS)
    total[:, 1] = 50 + np.arange(E)                               # one sample's totals all distinct
    total[:, 2] = rng.integers(0, 400, E)
    test = (total * rng.uniform(0.05, 0.6, size=(E, S))).astype(np.int64)
    ref = total - test
    # two cells no map holds: a total above the largest walked, and a sum below 0
    test[E - 2, 0], ref[E - 2, 0] = 7, max_total + 1 - 7
    test[E - 1, 0], ref[E - 1, 0] = -9, 4
    test[E - 2, 1], ref[E - 2, 1] = max_total, 0                  # the largest that is walked
    phi = np.array([0.2, 0.003, float("nan")])
    expected = np.array([0.5, 0.11, 0.3])
    return test.astype(np.int32), ref.astype(np.int32), phi, expected


def _element_wise(edlib, test, ref, phi, expected, seed, replicate, sample0=0):
    """the cohort draw restated cell by cell through the element-wise entries; skipped cells keep their counts"""
    E, S = test.shape
    out_t, out_r = test.copy(), ref.copy()
    mx = edlib.sim_geometry()["max_total"]
    for s in range(S):
        a, b = sc.shapes(phi[s], expected[s])
        if not (a > 0 and b > 0 and np.isfinite(a) and np.isfinite(b)):
            continue
        n = test[:, s].astype(np.int64) + ref[:, s]
        ok = (n >= 0) & (n <= mx)
        u = edlib.runif53(seed, np.arange(E), sample0 + s, replicate, 0)
        x = edlib.rbetabinom_ab_u(u[ok], n[ok], a, b)
        assert x.min() >= 0
        out_t[ok, s] = x
        out_r[ok, s] = n[ok] - x
    return out_t, out_r


def test_cohort_draw_is_the_element_wise_draw(edlib):
    mx = edlib.sim_geometry()["max_total"]
    test, ref, phi, expected = _cohort3(mx)
    E, S = test.shape
    plan = edlib.Plan([0, E], 1000 * np.arange(E), 1000 * np.arange(E) + 100)
    want_t, want_r = _element_wise(edlib, test, ref, phi, expected, SEED3, 1)
    for layout in (0, 1):
        t_in, r_in = (test, ref) if layout == 0 else (np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T))
        sim = plan.simulate(t_in, r_in, phi, expected, SEED3, replicate=1, layout=layout)
        got_t, got_r = _host(sim[0]), _host(sim[1])
        if layout:
            got_t, got_r = got_t.T, got_r.T
        assert got_t.dtype == np.int32 and got_t.shape == (E, S)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_r, want_r), layout
        assert np.array_equal(got_t.astype(np.int64) + got_r, test.astype(np.int64) + ref)           # every cell keeps its total
        # skipped cells are unchanged and counted: the two invalid totals and the whole sample with phi = NaN
        assert np.array_equal(got_t[:, 2], test[:, 2]) and np.array_equal(got_r[:, 2], ref[:, 2])
        assert (got_t[E - 2, 0], got_r[E - 2, 0]) == (7, mx + 1 - 7) and (got_t[E - 1, 0], got_r[E - 1, 0]) == (-9, 4)
        st = sim.stats()
        assert st["cells_skipped"] == E + 2 and st["cells_drawn"] == 2 * E - 2 and st["n_bad_samples"] == 1
        n_occ = sum(len(set((test[:, s].astype(np.int64) + ref[:, s])[(test[:, s].astype(np.int64) + ref[:, s] >= 0) &
                                                                      (test[:, s].astype(np.int64) + ref[:, s] <= mx)].tolist())) for s in range(S))
        assert st["n_jobs"] == n_occ
        assert 0 < st["tiles_walked"] <= st["tiles_full"]
        sim.free()
    # the draws did change the counts, and the 300 cells at n = 600 crossed in all three tiles of their walk
    assert np.mean(want_t[:, :2] != test[:, :2]) > 0.9
    x600 = want_t[(test[:, 0].astype(np.int64) + ref[:, 0]) == 600, 0]
    assert x600.size == 300 and (x600 < 256).any() and ((x600 >= 256) & (x600 < 512)).any() and (x600 >= 512).any()
    assert 0 <= want_t[E - 2, 1] <= mx
    plan.close()


def test_a_samples_draws_do_not_depend_on_the_call(edlib):
    """alone or as one of 3, 64 or 65 samples (with the matching sample0), in either layout, from host or device counts, replicate 2 asked
    alone or after replicates 0 and 1: identical bytes.  Two seeds differ, two replicates differ."""
    E, SF, g = 130, 65, 37
    rng = np.random.default_rng(21)
    total = rng.integers(0, 700, size=(E, SF))
    total[:, g] = np.where(np.arange(E) % 3 == 0, 120, total[:, g])            # (some totals shared, some alone)
    test = (total * rng.uniform(0.05, 0.5, size=(E, SF))).astype(np.int32)
    ref = (total - test).astype(np.int32)
    phi = rng.uniform(0.002, 0.05, SF)
    expected = rng.uniform(0.05, 0.4, SF)
    plan = edlib.Plan([0, 60, E], 1000 * np.arange(E), 1000 * np.arange(E) + 100)

    def column(lo, hi, layout=0, device=False, seed=77, replicate=2):
        t, r = test[:, lo:hi], ref[:, lo:hi]
        t, r = (np.ascontiguousarray(t), np.ascontiguousarray(r)) if layout == 0 else (np.ascontiguousarray(t.T), np.ascontiguousarray(r.T))
        keep = []
        if device:
            keep = [edlib.DeviceArray(t), edlib.DeviceArray(r)]
            t, r = keep
        sim = plan.simulate(t, r, phi[lo:hi], expected[lo:hi], seed, replicate=replicate, sample0=lo, layout=layout)
        gt, gr = _host(sim[0]), _host(sim[1])
        sim.free()
        for d in keep:
            d.free()
        if layout:
            gt, gr = gt.T, gr.T
        return np.ascontiguousarray(gt[:, g - lo]).tobytes() + np.ascontiguousarray(gr[:, g - lo]).tobytes()

    for r in (0, 1):
        column(g, g + 1, replicate=r)
    alone = column(g, g + 1)
    for lo, hi in ((g - 1, g + 2), (1, 65), (0, 65)):
        for layout in (0, 1):
            assert column(lo, hi, layout) == alone, (lo, hi, layout)
    assert column(g, g + 1, 1) == alone
    assert column(g, g + 1, 0, device=True) == alone and column(0, 65, 1, device=True) == alone
    assert column(g, g + 1, seed=78) != alone and column(g, g + 1, replicate=1) != alone
    assert column(g, g + 1, replicate=0) != column(g, g + 1, replicate=1)
    # the same counts under another global index are another sample: other draws
    t1, r1 = np.ascontiguousarray(test[:, g:g + 1]), np.ascontiguousarray(ref[:, g:g + 1])
    sim = plan.simulate(t1, r1, phi[g:g + 1], expected[g:g + 1], 77, replicate=2, sample0=g + 1)
    assert _host(sim[0])[:, 0].tobytes() + _host(sim[1])[:, 0].tobytes() != alone
    sim.free()
    plan.close()


def _pipeline_design():
    from exomedepth_amd import synth
    E, S = 2000, 6
    chrom_off = np.array([0, 1, 65, 130, E], dtype=np.int32)       # chains of 1, 64, 65 and the rest
    start = np.zeros(E, dtype=np.int32)
    for c in range(4):
        k = chrom_off[c + 1] - chrom_off[c]
        start[chrom_off[c]:chrom_off[c + 1]] = 20000 + 3000 * np.arange(k)
    end = (start + 200).astype(np.int32)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, 31, n_segments=3, mean_depth=90.0)
    return chrom_off, start, end, test, ref, phi, p


def test_null_call_table_is_the_pipeline_on_the_draws(edlib):
    chrom_off, start, end, test, ref, phi, p = _pipeline_design()
    E, S = test.shape
    out = edlib.null_call_table(chrom_off, start, end, test, ref, phi, p, 3, seed=606)
    fixed = edlib.null_call_table(chrom_off, start, end, test, ref, phi, p, [0, 1, 2], seed=606, refit=False)
    assert out["calls"].dtype == edlib.NULL_CALL_DTYPE and out["n_null_samples"] == 3 * S and out["phi"].shape == (3, S)
    assert np.array_equal(fixed["phi"], np.tile(phi, (3, 1))) and np.array_equal(fixed["expected"], np.tile(p, (3, 1)))
    plan = edlib.Plan(chrom_off, start, end)
    batch = edlib.Batch(plan, S)
    n_calls = 0
    for r in range(3):
        sim = plan.simulate(test, ref, phi, p, 606, replicate=r)
        th, rh = _host(sim[0]), _host(sim[1])                      # the replicate's draws copied out
        sim.free()
        assert np.array_equal(th.astype(np.int64) + rh, test.astype(np.int64) + ref) and np.mean(th != test) > 0.5
        dp, de = edlib.DeviceArray(np.zeros(S)), edlib.DeviceArray(np.zeros(S))
        batch.fit(th, rh, dp, de)
        batch.run(th, rh, dp, de)
        calls, info = batch.calls().copy(), batch.call_info().copy()
        mine = out["calls"][out["calls"]["replicate"] == r]
        assert len(mine) == len(calls)
        for k in calls.dtype.names:
            assert mine[k].tobytes() == calls[k].tobytes(), (r, k)
        for k in info.dtype.names:
            assert mine[k].tobytes() == info[k].tobytes(), (r, k)
        assert out["phi"][r].tobytes() == dp.to_host(np.float64, (S,)).tobytes()
        assert out["expected"][r].tobytes() == de.to_host(np.float64, (S,)).tobytes()
        n_calls += len(calls)
        batch.run(th, rh, phi, p)                                  # refit=False: run at the given parameters
        calls, info = batch.calls().copy(), batch.call_info().copy()
        mine = fixed["calls"][fixed["calls"]["replicate"] == r]
        assert len(mine) == len(calls)
        for k in calls.dtype.names:
            assert mine[k].tobytes() == calls[k].tobytes(), (r, k)
        assert mine["BF"].tobytes() == info["BF"].tobytes()
        dp.free(); de.free()
    batch.close()
    # the real calls against the null table
    batch = edlib.Batch(plan, S)
    batch.run(test, ref, phi, p)
    real, rinfo = batch.calls().copy(), batch.call_info().copy()
    batch.close(); plan.close()
    assert len(real) > 0
    null = out["calls"]
    got = edlib.false_calls_per_sample(rinfo["BF"], null["BF"], out["n_null_samples"], real["type"], null["type"])
    assert np.array_equal(got, sc.false_calls_loop(rinfo["BF"], null["BF"], out["n_null_samples"], real["type"], null["type"]))
    got = edlib.false_calls_per_sample(rinfo["BF"], null["BF"], out["n_null_samples"])
    assert np.array_equal(got, sc.false_calls_loop(rinfo["BF"], null["BF"], out["n_null_samples"]))
    print("null calls in 3 replicates x %d samples: %d (refit), %d (fixed); real calls %d" % (S, n_calls, len(fixed["calls"]), len(real)))


def test_planted_cells(edlib, oracle):
    """Planted cells equal rbetabinom_ab_u at the stream-1 uniforms and the shifted shapes, every other cell equals the unplanted draw;
    and the case chosen on the CPU (tests/test_simulate_host.py) is called on the GPU as the checker's draws and the oracle's CallCNVs
    call it, in every replicate.  No uniform of this input lies within the bar of a step: no cell is left out of the comparison."""
    case = sc.planted_case()
    chrom_off, start, end, test, ref, phi, expected, rows = case
    E, S = test.shape
    plan = edlib.Plan(chrom_off, start, end)
    planted = np.zeros((E, S), dtype=bool)
    for s in sc.PLANT_SAMPLES:
        planted[sc.PLANT_FIRST:sc.PLANT_LAST + 1, s] = True
    for r in range(sc.PLANT_REPLICATES):
        base = plan.simulate(test, ref, phi, expected, sc.PLANT_SEED, replicate=r)
        sim = plan.simulate(test, ref, phi, expected, sc.PLANT_SEED, replicate=r, plant=(rows, sc.PLANT_RATIO))
        bt, br, gt, gr = _host(base[0]), _host(base[1]), _host(sim[0]), _host(sim[1])
        assert sim.stats()["n_planted"] == 12 * 4 and base.stats()["n_planted"] == 0
        base.free(); sim.free()
        assert np.array_equal(gt[~planted], bt[~planted]) and np.array_equal(gr[~planted], br[~planted])
        assert np.array_equal(gt.astype(np.int64) + gr, test.astype(np.int64) + ref)
        ex = np.arange(sc.PLANT_FIRST, sc.PLANT_LAST + 1)
        for s in sc.PLANT_SAMPLES:
            a, b = sc.shapes(phi[s], sc.planted_prob(expected[s], sc.PLANT_RATIO))
            u = edlib.runif53(sc.PLANT_SEED, ex, s, r, 1)
            n = test[ex, s].astype(np.int64) + ref[ex, s]
            assert gt[ex, s].tolist() == edlib.rbetabinom_ab_u(u, n, a, b).tolist(), (r, s)
        assert np.mean(gt[planted] < bt[planted]) > 0.9            # half the copies: fewer test reads
        # the checker's own draws, cell for cell (nearest uniform to a step: far outside the bar, asserted on the CPU)
        want = sc.planted_draws(case, sc.PLANT_SEED, r, sc.PLANT_SAMPLES)
        for s in sc.PLANT_SAMPLES:
            assert np.array_equal(gt[:, s], want[s][0]), (r, s)
    plan.close()
    out = edlib.null_call_table(chrom_off, start, end, test, ref, phi, expected, sc.PLANT_REPLICATES, seed=sc.PLANT_SEED, refit=False,
                                plant=(rows, sc.PLANT_RATIO))
    for r in range(sc.PLANT_REPLICATES):
        want, nearest = sc.cpu_calls(case, oracle, sc.PLANT_SEED, r, sc.PLANT_SAMPLES)
        assert nearest > 1.0
        for s in sc.PLANT_SAMPLES:
            mine = out["calls"][(out["calls"]["replicate"] == r) & (out["calls"]["sample"] == s)]
            got = [(int(c["start_exon"]), int(c["end_exon"]), int(c["type"])) for c in mine]
            assert got == want[s], (r, s, got, want[s])
            assert (sc.PLANT_FIRST, sc.PLANT_LAST, 1) in got, (r, s, got)
    # a ratio that is not positive and finite is refused
    plan = edlib.Plan(chrom_off, start, end)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            plan.simulate(test, ref, phi, expected, 1, plant=(rows, bad))
    plan.close()


def test_per_sample_mirror_is_the_null_call_table_of_one_sample(edlib):
    import contextlib
    import io
    from exomedepth_amd import synth
    E = 1500
    chrom_off, start, end = synth.exon_design(E, 3, 12)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, 1, 12, n_segments=2, mean_depth=120.0)
    chrom = np.repeat(["1", "2", "3"], np.diff(chrom_off))
    with contextlib.redirect_stdout(io.StringIO()):
        x = edlib.ExomeDepth(test[:, 0].astype(float), ref[:, 0].astype(float), phi=float(phi[0]), expected=float(p[0]))
    got = x.null_calls(chrom, start, end, replicates=2, seed=5)
    want = edlib.null_call_table(chrom_off, start, end, test, ref, phi[:1], p[:1], 2, seed=5)
    assert got["calls"].tobytes() == want["calls"].tobytes() and got["n_null_samples"] == 2
    assert got["phi"].tobytes() == want["phi"].tobytes() and got["phi"].shape == (2, 1)
    assert not np.array_equal(got["phi"][0], got["phi"][1])         # each replicate's own fit


def test_refusals_enqueue_nothing(edlib):
    from exomedepth_amd import _lib
    L = _lib.lib()
    E, S = 40, 3
    rng = np.random.default_rng(2)
    test = rng.integers(0, 50, size=(E, S)).astype(np.int32)
    ref = rng.integers(50, 200, size=(E, S)).astype(np.int32)
    phi, expected = np.full(S, 0.01), np.full(S, 0.2)
    plan = edlib.Plan([0, E], 1000 * np.arange(E), 1000 * np.arange(E) + 100)
    good = plan.simulate(test, ref, phi, expected, 5)              # a draw that works, so that the stats have something to keep
    stats0 = good.stats()
    good.free()
    dt, dr = edlib.DeviceArray(test), edlib.DeviceArray(ref)
    sentinel = np.full((E, S), -77, dtype=np.int32)
    ot, orr = edlib.DeviceArray(sentinel), edlib.DeviceArray(sentinel)
    pp, pe = phi.ctypes.data_as(C.c_void_p), expected.ctypes.data_as(C.c_void_p)

    def call(plan_h=plan.handle, t=dt.ptr, r=dr.ptr, ph=pp, ex=pe, n=S, s0=0, layout=0, rep=0, o1=ot.ptr, o2=orr.ptr):
        return L.ed_plan_simulate(plan_h, t, r, ph, ex, n, s0, layout, 5, rep, o1, o2, None)

    def last_stats():
        cnt, ms = (C.c_int64 * 6)(), (C.c_double * 3)()
        assert L.ed_sim_stats(cnt, ms) == 0
        return list(cnt), list(ms)

    before = last_stats()
    assert before[0][3] == stats0["cells_drawn"] == E * S
    inside = C.c_void_p(dt.ptr.value + 4 * (E * S - 1))            # overlaps the last cell of test
    refused = [dict(plan_h=None), dict(t=None), dict(r=None), dict(ph=None), dict(ex=None), dict(o1=None), dict(o2=None), dict(layout=2),
               dict(layout=-1), dict(n=0), dict(n=(1 << 20) + 1), dict(rep=-1), dict(s0=-1), dict(o1=dt.ptr), dict(o2=dr.ptr), dict(o1=dr.ptr),
               dict(o2=inside), dict(o1=orr.ptr)]
    for kw in refused:
        assert call(**kw) == -1, kw                                # ED_ERR_INVALID
        assert L.ed_last_error()
    assert last_stats() == before                                  # no kernel time was taken
    assert np.array_equal(ot.to_host(), sentinel) and np.array_equal(orr.to_host(), sentinel)
    assert np.array_equal(dt.to_host(), test) and np.array_equal(dr.to_host(), ref)
    # listed cells: the same refusals, and a cell outside the counts
    ce, cs = np.array([0, E], dtype=np.int32), np.array([0, 0], dtype=np.int32)
    ab = np.array([1.0, 1.0])
    p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.ed_plan_simulate_cells(plan.handle, dt.ptr, dr.ptr, p(ce), p(cs), p(ab), p(ab), 2, S, 0, 0, 5, 0, 1, ot.ptr, orr.ptr, None) != 0
    assert L.ed_plan_simulate_cells(plan.handle, dt.ptr, dr.ptr, p(ce), p(cs), p(ab), p(ab), 1, S, 0, 0, 5, -1, 1, ot.ptr, orr.ptr, None) != 0
    assert L.ed_plan_simulate_cells(plan.handle, dt.ptr, dr.ptr, p(ce), p(cs), p(ab), p(ab), 1, S, 0, 0, 5, 0, 1, dt.ptr, orr.ptr, None) != 0
    assert np.array_equal(ot.to_host(), sentinel) and np.array_equal(orr.to_host(), sentinel)
    assert call() == 0                                             # and the same arguments unbroken do draw
    got = ot.to_host()
    assert not np.array_equal(got, sentinel) and np.array_equal(got.astype(np.int64) + orr.to_host(), test.astype(np.int64) + ref)
    # the other entries' refusals
    assert L.ed_sim_stats(None, None) != 0 and L.ed_sim_geometry(None) != 0
    assert L.ed_runif53(1, None, None, None, 0, 4, None) != 0 and L.ed_rbetabinom_ab_u(None, None, None, None, 4, None) != 0
    assert L.ed_runif53(1, None, None, None, 0, -1, None) != 0
    with pytest.raises(ValueError):
        edlib.runif53(1, [-1], 0, 0)
    with pytest.raises(ValueError):
        edlib.runif53(2 ** 64, [1], 0, 0)
    for d in (dt, dr, ot, orr):
        d.free()
    plan.close()
