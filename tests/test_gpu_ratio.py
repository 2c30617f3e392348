"""The copy-ratio profile on the GPU (csrc/edratio.inc: k_ratio_profile, k_ratio_sum) against the checker (tests/ratio_checker.py), bit
for bit against itself, anchored to the call decoration's Bayes factor, its refusals, and CallCNVs(copy_number=True) on the bundled counts.

The bar (derived in the checker's docstring): |dev - fsum| <= 2^-52 |fsum| + n 2^-100 sum |t_i| per value -- one rounding of the exact sum
plus the double-double's carry; NaN is compared for NaN; no value is excused.  With the rounding's remainder beside it (tail=True) a
value is held to the carry alone, in exact arithmetic: |dev + tail - sum| <= n 2^-100 sum |t_i|.

Shapes: a plan of 4 chromosomes of 1, 65, 130 and 513 exons, 7 samples.  Rows of 1, 2, 4, 5, 63, 64, 65, 128 and 129 exons, every whole
chromosome, rows one short of, on and one beyond a segment (ratio_geometry), rows at a chain's first and last exon, two overlapping rows
of one sample; 16 doses per row from -1.9 to 2 with 0 and +-1, a NaN and doses outside (-2, 2]; a sample whose phi makes a1 <= 0 at the
lowest ratio.  One reference is computed for all rows x 16 doses and shared: a value depends on its row and its dose alone, so every
narrower case is a slice.

Measured on an MI355X when this file was written (test_report prints the figures with -s): see DESIGN.md 4.23.
"""
import os

import numpy as np
import pytest

import mixture_checker as mc
import ratio_checker as rc

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 130, 513)
S = 7
LOG10E = 0.43429448190325182765
REPORT = {"values": 0, "frac": 0.0, "nan": 0, "anchor": 0.0, "anchor_rounded": 0.0, "calls": 0, "ratio_gap": None, "tail": 0.0}
_CACHE = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _case(edlib, oracle):
    if "case" not in _CACHE:
        geo = edlib.ratio_geometry()
        seg = geo["seg_tiles"] * 64
        rng = np.random.default_rng(29)
        chrom_off, start, end, test, ref, _, _ = mc.draw(SIZES, [(1.0, None, 0.5, 1.0, 0.3, None, 1.0)[s] for s in range(S)], 31, depth=300.0)
        E = test.shape[0]
        for s in range(S):                                      # cells without test reads, and cells without reads at all
            cells = rng.choice(E, 10, replace=False)
            test[cells[:5], s] = 0
            test[cells[5:], s], ref[cells[5:], s] = 0, 0
        phi = rng.uniform(5e-4, 3e-3, S)
        expected = rng.uniform(0.30, 0.55, S)
        phi[6], expected[6] = 0.2, 0.4                          # a1 <= 0 at the lowest ratios: ep (1 - ep) <= phi e (1 - e)
        lo3, hi3 = int(chrom_off[3]), int(chrom_off[4])         # the chromosome of 513 exons
        rows = []
        for j, n in enumerate((1, 2, 4, 5, 63, 64, 65, 128, 129)):
            a = lo3 + 7 * j + (j % 3)
            rows.append((j % S, 3, a, a + n - 1))
        for c in range(4):                                      # whole chromosomes (the first is a chain of one exon)
            rows.append(((c + 2) % S, c, int(chrom_off[c]), int(chrom_off[c + 1]) - 1))
        for n in (seg - 1, seg, seg + 1):                       # around a segment
            if n <= hi3 - lo3:
                rows.append((n % S, 3, hi3 - n, hi3 - 1))
                rows.append(((n + 3) % S, 3, lo3, lo3 + n - 1))
        rows += [(1, 2, int(chrom_off[2]), int(chrom_off[2])), (1, 2, int(chrom_off[3]) - 1, int(chrom_off[3]) - 1),     # a chain's first and last exon
                 (4, 3, lo3, lo3 + 4), (4, 3, hi3 - 5, hi3 - 1),
                 (5, 3, lo3 + 100, lo3 + 180), (5, 3, lo3 + 150, lo3 + 300),                                           # overlapping, one sample
                 (6, 3, lo3 + 40, lo3 + 75), (6, 1, int(chrom_off[1]) + 3, int(chrom_off[1]) + 60)]                    # the sample of the large phi
        R = np.zeros(len(rows), dtype=edlib.CALL_DTYPE)
        for i, (s, c, a, b) in enumerate(rows):
            R[i] = (s, c, a, b, 1 + i % 2, b - a + 1)
        n = R.size
        # ratios, as the interface takes them; the doses are what it makes of them: -1.9 .. 2 with 0 and +-1, a NaN, doses outside (-2, 2]
        base = np.array([0.05, 0.25, 0.5, 0.75, 1.0, 1.125, 1.5, 1.75, 2.0, np.nan, 2.25, 0.0, 0.85, 1.35, 1.95, 0.05])
        ratios = np.repeat(base[:, None], n, axis=1)
        ratios[12:15, :] = rng.uniform(0.05, 2.0, (3, n))        # every row its own ratios
        ratios[10, 1::2] = np.inf
        ratios[11, 2::3] = -2.5
        doses = 2.0 * (ratios - 1.0)
        assert doses[2, 0] == -1.0 and doses[4, 0] == 0.0 and doses[6, 0] == 1.0 and doses[8, 0] == 2.0 and doses[11, 0] == -2.0
        terms = {}
        want, bar = rc.profile(oracle, R, test, ref, phi, expected, doses, terms_out=terms)
        assert np.isnan(want[9:12]).all() and np.isfinite(want[[0, 2, 4, 6, 8]][:, R["sample"] != 6]).all()
        _CACHE["case"] = dict(geo=geo, seg=seg, chrom_off=chrom_off, start=start, end=end, test=test, ref=ref, phi=phi, expected=expected,
                              rows=R, ratios=ratios, doses=doses, want=want, bar=bar, terms=terms)
    return _CACHE["case"]


def _run(edlib, k, rows=None, ratios=None, layout=0, samples=None, tail=False):
    """L (G, n_rows) of the device for rows x ratios; samples: the columns of the counts that are handed over (rows index into them);
    tail: (L, L_tail) of the entry that returns the roundings' remainders"""
    rows = k["rows"] if rows is None else rows
    ratios = k["ratios"] if ratios is None else ratios
    cols = np.arange(S) if samples is None else np.asarray(samples)
    test, ref = np.ascontiguousarray(k["test"][:, cols]), np.ascontiguousarray(k["ref"][:, cols])
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    try:
        L, used, *rest = plan.ratio_profile(rows, test, ref, k["phi"][cols], k["expected"][cols], np.ascontiguousarray(ratios.T), layout=layout,
                                            tail=tail)
    finally:
        plan.close()
    assert np.array_equal(bits(used.T), bits(1.0 + (2.0 * (ratios - 1.0)) / 2.0))     # the ratio its dose stands for
    if tail:
        return np.ascontiguousarray(L.T), np.ascontiguousarray(rest[0].T)
    return np.ascontiguousarray(L.T)


def _base(edlib, k):
    if "base" not in _CACHE:
        _CACHE["base"] = _run(edlib, k)
    return _CACHE["base"]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("G", [1, 16])
def test_against_the_checker(edlib, oracle, G, layout):
    k = _case(edlib, oracle)
    got = _run(edlib, k, ratios=k["ratios"][:G], layout=layout)
    want, bar = k["want"][:G], k["bar"][:G]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), np.argwhere(np.isnan(got) != np.isnan(want))
    fin = ~np.isnan(want)
    dev = np.abs(got[fin].astype(np.longdouble) - want[fin].astype(np.longdouble)).astype(np.float64)
    frac = dev / bar[fin]
    print("G = %d, layout %d: %d values, %d NaN, largest share of the bar %.4f" % (G, layout, fin.sum(), (~fin).sum(), frac.max()))
    REPORT["values"] += int(fin.sum())
    REPORT["nan"] += int((~fin).sum())
    REPORT["frac"] = max(REPORT["frac"], float(frac.max()))
    assert np.all(dev <= bar[fin]), float(frac.max())
    if G == 16:
        big = k["rows"]["sample"] == 6
        print("the sample of phi = 0.2 at dose -1.9: device", got[0, big], "checker", want[0, big])
        assert np.array_equal(bits(got[0]), bits(got[15]))                  # the same dose at the grid's two ends


def test_bit_invariance(edlib, oracle):
    k = _case(edlib, oracle)
    base = _base(edlib, k)
    R, ratios = k["rows"], k["ratios"]
    n = R.size
    # shuffled
    perm = np.random.default_rng(5).permutation(n)
    assert np.array_equal(bits(_run(edlib, k, rows=R[perm], ratios=ratios[:, perm])), bits(base[:, perm]))
    # alone against among others
    for i in range(n):
        assert np.array_equal(bits(_run(edlib, k, rows=R[i:i + 1], ratios=ratios[:, i:i + 1])), bits(base[:, i:i + 1])), i
    # the sample extracted (S = 1) against S = 7
    for s in range(S):
        mine = np.flatnonzero(R["sample"] == s)
        alone = R[mine].copy()
        alone["sample"] = 0
        assert np.array_equal(bits(_run(edlib, k, rows=alone, ratios=ratios[:, mine], samples=[s])), bits(base[:, mine])), s
    # layout 1 against layout 0
    assert np.array_equal(bits(_run(edlib, k, layout=1)), bits(base))
    # the grid reversed: a dose at index g against index 15 - g
    assert np.array_equal(bits(_run(edlib, k, ratios=ratios[::-1])), bits(base[::-1]))
    # G = 1 against G = 16, every column on its own
    for g in (0, 4, 8, 13):
        assert np.array_equal(bits(_run(edlib, k, ratios=ratios[g:g + 1])), bits(base[g:g + 1])), g


def test_the_tail_completes_the_sum(edlib, oracle):
    """tail=True: the same values to the bit, and beside each what its rounding dropped -- value + tail is the exact sum of the checker's
    terms up to the double-double's carry, n 2^-100 sum |t_i| (exact rational arithmetic; every finite value of the case), 0 beside a
    value that is not finite; and the tails are as invariant as the values"""
    k = _case(edlib, oracle)
    base = _base(edlib, k)
    R, ratios = k["rows"], k["ratios"]
    L, T = _run(edlib, k, tail=True)
    assert np.array_equal(bits(L), bits(base))
    fin = np.isfinite(L)
    assert np.all(T[~fin] == 0.0) and np.all(np.isfinite(T))
    assert np.array_equal(L[fin] + T[fin], L[fin]) and np.all(np.abs(T[fin]) <= 0.5 * np.spacing(np.abs(L[fin])))
    assert set(k["terms"]) == set(zip(*np.nonzero(~np.isnan(k["want"]))))
    worst = 0.0
    for (g, r), t in k["terms"].items():
        gap, carry = rc.tail_gap(t, L[g, r], T[g, r])
        assert gap <= carry, (g, r, gap, carry)
        worst = max(worst, gap / carry)
    REPORT["tail"] = worst
    print("%d values with their tails: largest |value + tail - exact sum| is %.3g of the carry's bar; %d tails are not 0" % (
        len(k["terms"]), worst, int((T != 0).sum())))
    assert (T != 0).sum() > len(k["terms"]) // 4                                       # (the tails are there: a sum of n > 1 terms rarely is a double)
    perm = np.random.default_rng(6).permutation(R.size)
    assert np.array_equal(bits(_run(edlib, k, rows=R[perm], ratios=ratios[:, perm], tail=True)[1]), bits(T[:, perm]))
    assert np.array_equal(bits(_run(edlib, k, layout=1, tail=True)[1]), bits(T))
    assert np.array_equal(bits(_run(edlib, k, ratios=ratios[::-1], tail=True)[1]), bits(T[::-1]))
    for i in (0, 8, R.size - 1):
        assert np.array_equal(bits(_run(edlib, k, rows=R[i:i + 1], ratios=ratios[4:5, i:i + 1], tail=True)[1]), bits(T[4:5, i:i + 1])), i


def _anchor(edlib, oracle):
    """a strict run at mixture 1 on the case's first six samples (not the one of phi = 0.2): its calls, their decoration, their profile at
    the ratios 0.5, 1, 1.5 -- computed once, shared"""
    if "anchor" not in _CACHE:
        k = _case(edlib, oracle)
        cols = np.arange(6)
        test, ref = np.ascontiguousarray(k["test"][:, cols]), np.ascontiguousarray(k["ref"][:, cols])
        plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
        batch = edlib.Batch(plan, cols.size)
        try:
            batch.enable_timing()
            batch.run(test, ref, k["phi"][cols], k["expected"][cols], mixture=1.0)
            calls, info = batch.calls(), batch.call_info()
            L, used = batch.call_ratio_profile([0.5, 1.0, 1.5])
            ms = batch.call_ratio_ms()
            L3, used3, T = batch.call_ratio_profile([0.5, 1.0, 1.5], tail=True)                                    # ... with the roundings' remainders
            L2, _, T2 = plan.ratio_profile(calls, test, ref, k["phi"][cols], k["expected"][cols], [0.5, 1.0, 1.5], tail=True)   # the same rows through the plan's entry
        finally:
            batch.close()
            plan.close()
        assert np.array_equal(bits(L3), bits(L)) and np.array_equal(bits(used3), bits(used)) and np.array_equal(bits(T2), bits(T))
        Lt = np.where(calls["type"] == 1, L[:, 0], L[:, 2])
        Tt = np.where(calls["type"] == 1, T[:, 0], T[:, 2])
        _CACHE["anchor"] = dict(calls=calls, info=info, L=L, used=used, ms=ms, L2=L2, Lt=Lt, T=T, bf_rounded=LOG10E * (Lt - L[:, 1]),
                                bf=LOG10E * ((Lt - L[:, 1]) + (Tt - T[:, 1])))
    return _CACHE["anchor"]


def test_anchored_to_the_call_decoration(edlib, oracle):
    """The batch's entry and the plan's give a call the same bits, and log10(e) (L(the call's type) - L(1)) of the values rounded to one
    double each is the call's BF_raw to what two sums rounded to a double can carry.  Every term is <= 0, so |L| is the sum of its terms' sizes: each L is within 2^-53 |L| of its
    exact sum, BF_raw's per-term differences are within 2^-53 (|L(type)| + |L(1)|) of theirs, and the products and the subtraction round
    BF by 2^-52 more: |BF - BF_raw| <= log10(e) 2^-52 (|L(type)| + |L(1)|) + 2 * 2^-52 |BF_raw|.  (Measured: at most 0.354 of that.)"""
    a = _anchor(edlib, oracle)
    calls, info, L = a["calls"], a["info"], a["L"]
    assert calls.size > 0 and L.shape == (calls.size, 3) and np.array_equal(a["used"], np.repeat([[0.5, 1.0, 1.5]], calls.size, axis=0))
    assert np.array_equal(bits(L), bits(a["L2"])) and a["ms"] > 0.0
    dev = np.abs(a["bf_rounded"] - info["BF_raw"])
    REPORT["anchor_rounded"] = float((dev / np.abs(info["BF_raw"])).max() * 2.0 ** 52)
    own = LOG10E * 2.0 ** -52 * (np.abs(a["Lt"]) + np.abs(L[:, 1])) + 2 * 2.0 ** -52 * np.abs(info["BF_raw"])
    print("%d calls, largest share of the rounding of the two sums %.3f (profile kernels %.3f ms)" % (calls.size, (dev / own).max(), a["ms"]))
    assert np.all(np.isfinite(info["BF_raw"])) and np.all(dev <= own), float((dev / own).max())


def test_anchored_to_the_call_decoration_at_the_issue_s_bound(edlib, oracle):
    """The bound the feature's issue sets: log10(e) (L(type) - L(1)) of Batch.call_ratio_profile([0.5, 1, 1.5]) is BF_raw within
    4 * 2^-52 |BF_raw|, for every call.

    Two values rounded to ONE double each cannot carry that: a strict term is the log of a probability without its binomial coefficient,
    about -200 per exon at 300 reads, so |L(type)| + |L(1)| is some 150 times their difference and the subtraction cancels seven bits
    (the test above holds the rounded values to what they can carry; 53.5 x 2^-52 was measured on these calls).  So the comparison is
    made on the sums as the kernel holds them, value + tail (tail=True):  BF = log10(e) ((L(type) - L(1)) + (tail(type) - tail(1))).
    The terms are BF_raw's and both sides add them as double-doubles (carry <= n 2^-100 sum |t_i|, test_the_tail_completes_the_sum), so
    what is left is the rounding of the two subtractions, their sum and the product here, and of the sum and the product there."""
    a = _anchor(edlib, oracle)
    calls, info, L = a["calls"], a["info"], a["L"]
    rel = np.abs(a["bf"] - info["BF_raw"]) / np.abs(info["BF_raw"])
    w = int(np.argmax(rel))
    print("%d calls, largest |BF - BF_raw| / |BF_raw| = %.3g = %.3f x 2^-52 at call %d (%d exons, BF_raw %.4f, L(type) %.3f, L(1) %.3f); %d calls beyond "
          "4 x 2^-52, %d equal to the bit" % (calls.size, rel.max(), rel.max() * 2.0 ** 52, w, calls["nexons"][w], info["BF_raw"][w], a["Lt"][w], L[w, 1],
                                               int((rel > 4 * 2.0 ** -52).sum()), int((rel == 0).sum())))
    REPORT["anchor"], REPORT["calls"] = float(rel.max() * 2.0 ** 52), int(calls.size)
    assert np.all(rel <= 4 * 2.0 ** -52), rel.max() * 2.0 ** 52


def test_refusals(edlib, oracle):
    from exomedepth_amd import synth
    k = _case(edlib, oracle)
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    test, ref = np.ascontiguousarray(k["test"]), np.ascontiguousarray(k["ref"])
    good = k["rows"][:3]
    try:
        L, used = plan.ratio_profile(good[:0], test, ref, k["phi"], k["expected"], [0.5, 1.0])          # no rows: a success that does nothing
        assert L.shape == (0, 2) and used.shape == (0, 2)
        for G in (0, 17):
            with pytest.raises(edlib.EdError, match=r"G = %d is outside 1 \.\. 16.*status -1" % G):
                plan.ratio_profile(good, test, ref, k["phi"], k["expected"], np.ones(G))
        E, C3 = int(k["chrom_off"][-1]), int(k["chrom_off"][3])
        for field, value in (("sample", S), ("sample", -1), ("chrom", 4), ("chrom", -1), ("start_exon", C3 - 1), ("end_exon", E),
                             ("end_exon", int(good[1]["start_exon"]) - 1)):
            bad = good.copy()
            bad[field][1] = value
            with pytest.raises(edlib.EdError, match=r"row 1 does not lie inside.*status -1"):
                plan.ratio_profile(bad, test, ref, k["phi"], k["expected"], [1.0])
        with pytest.raises(edlib.EdError, match="layout"):
            plan.ratio_profile(good, test.T.copy(), ref.T.copy(), k["phi"], k["expected"], [1.0], layout=2)
    finally:
        plan.close()
    # the batch's entry after a depth-binned and after a covariate run: ED_ERR_STATE; after a plain run on the same batch it serves again
    E2, S2, B = 4000, 5, 4
    chrom_off, start, end = synth.exon_design(E2, 4, 95)
    t2, r2, _, _, _ = synth.counts_numpy(chrom_off, S2, 95, n_segments=3, mean_depth=60.0)
    plan = edlib.Plan(chrom_off, start, end)
    batch = edlib.Batch(plan, S2)
    try:
        with pytest.raises(edlib.EdError, match="status -5"):
            batch.call_ratio_profile([1.0])                                                              # nothing has run
        dphib, dedges, dexp = edlib.DeviceArray(np.zeros((B, S2))), edlib.DeviceArray(np.zeros((B + 1, S2))), edlib.DeviceArray(np.zeros(S2))
        batch.fit_bins(t2, r2, B, dphib, dedges, dexp)
        batch.run_bins(t2, r2, B, dphib, dedges, dexp)
        assert batch.n_calls() > 0
        with pytest.raises(edlib.EdError, match="depth-binned or covariate.*status -5"):
            batch.call_ratio_profile([0.5, 1.0])
        X = np.random.default_rng(3).normal(0.0, 1.0, (E2, 1))
        dbeta, dphi = edlib.DeviceArray(np.zeros((2, S2))), edlib.DeviceArray(np.zeros(S2))
        batch.fit_cov(t2, r2, X, dbeta, dphi)
        batch.run_cov(t2, r2, X, dbeta, dphi)
        with pytest.raises(edlib.EdError, match="depth-binned or covariate.*status -5"):
            batch.call_ratio_profile([0.5, 1.0])
        info = batch.call_info()                                                                         # the batch is as it was
        assert info.size == batch.n_calls()
        batch.run(t2, r2, dphi, dexp)
        L, _ = batch.call_ratio_profile([0.5, 1.0])
        assert L.shape == (batch.n_calls(), 2) and np.all(np.isfinite(L))
        with pytest.raises(edlib.EdError, match=r"G = 17 is outside"):
            batch.call_ratio_profile(np.ones(17))
    finally:
        batch.close()
        plan.close()


def test_callcnvs_copy_number_on_the_bundled_counts(edlib):
    d = np.load(os.path.join(GOLDEN, "exomecount_chr1.npz"))
    start, end, counts = d["start"], d["end"], d["counts"].astype(np.float64)
    n = start.size
    chrom, names = ["chr1"] * n, ["exon%d" % i for i in range(n)]
    test, ref = counts[:, 0], counts.sum(axis=1) - counts[:, 0]
    x = edlib.ExomeDepth(test, ref)
    plain = [dict(c) for c in x.CallCNVs(chrom, start, end, names).CNV_calls]
    withcn = x.CallCNVs(chrom, start, end, names, copy_number=True).CNV_calls
    new = ("copy.ratio", "copy.ratio.lo", "copy.ratio.hi", "copy.number", "BF.copy.number", "mosaic.gain")
    assert len(plain) == len(withcn) > 0
    gap = 0.0
    for a, b in zip(plain, withcn):
        assert list(b)[:len(a)] == list(a) and list(b)[len(a):] == list(new)
        assert all(b[key] == a[key] for key in a)
        assert b["copy.ratio.lo"] <= b["copy.ratio"] <= b["copy.ratio.hi"]
        assert 0 <= b["copy.number"] <= 4 and b["BF.copy.number"] >= 0.0 and b["mosaic.gain"] >= 0.0
        print("%-28s %-11s nexons %3d reads.ratio %.3f copy.ratio %.4f [%.4f, %.4f] CN %d (BF %.2f) mosaic.gain %.2f" % (
            b["id"], b["type"], b["nexons"], b["reads.ratio"], b["copy.ratio"], b["copy.ratio.lo"], b["copy.ratio.hi"], b["copy.number"],
            b["BF.copy.number"], b["mosaic.gain"]))
        if np.isfinite(b["reads.ratio"]):
            gap = max(gap, abs(b["copy.ratio"] - b["reads.ratio"]))
    REPORT["ratio_gap"] = gap
    print("largest |copy.ratio - reads.ratio| over %d calls: %.4f" % (len(plain), gap))


def test_report():
    print("copy-ratio profile: %(values)d values and %(nan)d NaN against the checker, largest share of the bar %(frac).4f; %(calls)d calls "
          "anchored to BF_raw within %(anchor).3f x 2^-52 (the rounded values alone: %(anchor_rounded).1f x 2^-52), value + tail within %(tail).3g of "
          "the carry's bar; largest |copy.ratio - reads.ratio| %(ratio_gap)s" % REPORT)
