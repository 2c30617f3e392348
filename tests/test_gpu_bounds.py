"""Breakpoint credible intervals on the GPU (csrc/edbounds.inc: k_call_bounds) against the long-double checker (tests/bounds_checker.py)
evaluated on the device's own likelihood matrix.

The three doubles of a row are held to a derived bar: 4 posterior_checker.bar(m, alpha) of the chain (two beta and two log gamma in the
worst case) + 2^-50 (n + 1) max(1, max |partial sum|) for a walk of n steps.  The four bounds must equal the checker's; a bound may
differ only if every exon between the two has |G_checker - threshold| within that bar, and at most 1 % of the (row, bound) pairs of a
test may use that excuse (tests/test_bounds_host.py asserts that the checker alone stays within it).

The anchor is asserted against the device's OWN log gamma (Batch.posterior(log=True), Posterior.log_posterior()), with no tolerance: for
every row that is not flagged, anchor_exon is the first arg-max, NaN ignored, of those values over start_exon .. end_exon, and log_anchor
is that entry bit for bit; test_anchor_rule_on_planted_ties plants exact ties and NaN in the device array itself.  The checker then walks
from that anchor, at the bars above.  That the device's anchor is also the long-double arg-max up to the posterior's error is asserted
for every row as a bound: the checker's log gamma at the device's anchor lies within 2 posterior_checker.bar of the checker's largest
(each of the two values carries up to one bar).  Where a call is certain several exons of a row have gamma = 1 to the last bits, so the
two arg-max do fall on different exons there; how often is reported.

Measured on an MI355X when this file was written (test_report prints the figures with -s): see DESIGN.md 4.20.
"""
import types

import numpy as np
import pytest

import bounds_checker as bc
import posterior_checker as pc
from exomedepth_amd.api import CALL_BOUNDS_DTYPE, CALL_DTYPE
from test_gpu_chain_geometry import LOUD, SETTINGS
from test_gpu_posterior import Layout, _counts, _layout

pytestmark = pytest.mark.gpu

S_MAX = 130
WIDTHS = (1, 3, 16, 17, 64, 65, 130)
LEVELS = (0.5, 0.95)
NEST = (0.5, 0.8, 0.95, 0.999)
BOUNDS = ("start_lo", "start_hi", "end_lo", "end_hi")
DOUBLES = ("log_anchor", "log_keep_start", "log_keep_end")
REPORT = {"rows": 0, "pairs": 0, "excused": 0, "ties": 0, "flagged": 0, "frac": 0.0, "longest": 0, "width0": 0, "widths": 0, "wmax": 0}
_CACHE = {}


def _plan(edlib, L, setting):
    tp, ln = SETTINGS[setting]
    return edlib.Plan(L.chrom_off, L.start, L.end, tp, ln), pc.transitions(L.chrom_off, L.start, L.end, tp, ln)


def _rows(sample, chrom, start, end, type_):
    r = np.zeros(len(sample), dtype=CALL_DTYPE)
    r["sample"], r["chrom"], r["start_exon"], r["end_exon"], r["type"] = sample, chrom, start, end, type_
    r["nexons"] = r["end_exon"] - r["start_exon"] + 1
    return r


def _check_flagged(r, q):
    assert q["flags"] == 1 and all(np.isnan(q[k]) for k in DOUBLES), (r, q)
    assert (q["anchor_exon"], q["start_lo"], q["start_hi"]) == (r["start_exon"],) * 3 and (q["end_lo"], q["end_hi"]) == (r["end_exon"],) * 2, (r, q)


def _device_anchor(dlp, r):
    """the anchor by the rule, from the device's own log gamma (E, 2, S): (exon, value) of the first arg-max over the row, NaN ignored;
    None for another type or when no value of the row is finite"""
    if int(r["type"]) not in (1, 2):
        return None
    lg = dlp[int(r["start_exon"]):int(r["end_exon"]) + 1, int(r["type"]) - 1, int(r["sample"])]
    v = np.where(np.isnan(lg), -np.inf, lg)
    k = int(np.argmax(v))                                 # the first of equal maxima
    return (int(r["start_exon"]) + k, lg[k]) if np.isfinite(v[k]) else None


def _check_anchor(r, q, da):
    """no tolerance: the flag, the anchor and log_anchor follow from the device's own log gamma"""
    if da is None:
        _check_flagged(r, q)
        return
    assert q["flags"] == 0 and int(q["anchor_exon"]) == da[0], (r, q, da)
    assert bits(q["log_anchor"]) == bits(da[1]), (r, q, da)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _verify(L, trs, want, ll, dlp, rows, got, levels=LEVELS):
    """device records got[level] of the rows against the device's own log gamma dlp (E, 2, S) -- flag, anchor, log_anchor -- and against
    the checker on ll (E, 3, S), walking from that anchor; want = pc.run(ll) at long double.  Returns the number of (row, bound) pairs and
    of those excused; updates REPORT."""
    pairs = excused = 0
    for c in np.unique(rows["chrom"]):
        c = int(c)
        lo, m = int(L.chrom_off[c]), L.sizes[c]
        sel = np.flatnonzero(rows["chrom"] == c)
        res, block = want[c], ll[lo:lo + m]
        bar_post = pc.bar(m, res["alpha"])
        anchors = [_device_anchor(dlp, rows[n]) for n in sel]
        specs = [(int(rows["start_exon"][n]) - lo, int(rows["end_exon"][n]) - lo, int(rows["type"][n]), int(rows["sample"][n])) +
                 (() if da is None else (da[0] - lo,)) for n, da in zip(sel, anchors)]
        recs = bc.rows(res, block, trs[c], specs, levels)
        for i, n in enumerate(sel):
            rec, da = recs[i], anchors[i]
            assert (rec is None) == (da is None), (c, specs[i])
            if rec is not None:
                # the device's anchor is the long-double arg-max up to the posterior's error: a bound, asserted for every row
                r0, r1, t, s = specs[i][:4]
                own, lg_own = bc.anchor(res, r0, r1, t, s)
                assert float(lg_own - res["log_gamma"][rec["anchor"], t, s]) <= 2.0 * bar_post[s], (c, specs[i], own)
                REPORT["ties"] += int(own != rec["anchor"])
            for level in levels:
                q = got[level][n]
                _check_anchor(rows[n], q, da)
                if rec is None:
                    REPORT["flagged"] += 1
                    continue
                a = rec["anchor"]
                b = [int(q[k]) - lo for k in BOUNDS]
                assert 0 <= b[0] <= b[1] <= a <= b[2] <= b[3] < m, (c, specs[i], level, q)
                for which in range(4):
                    pairs += 1
                    if b[which] != rec["bounds"][level][which]:
                        assert bc.excused(rec, level, which, b[which]), (c, specs[i], level, BOUNDS[which], b[which], rec["bounds"][level])
                        excused += 1
                for name, bar in (("log_anchor", rec["bar_anchor"]), ("log_keep_start", rec["bar_keep_start"]), ("log_keep_end", rec["bar_keep_end"])):
                    w, g = rec[name], q[name]
                    if np.isneginf(float(w)):
                        assert np.isneginf(g), (c, specs[i], level, name, g)
                        continue
                    d = abs(float(np.longdouble(g) - w))
                    assert d <= bar, (c, specs[i], level, name, float(g), float(w), d, bar)
                    REPORT["frac"] = max(REPORT["frac"], d / bar)
                REPORT["longest"] = max(REPORT["longest"], a - b[0], b[3] - a)
                REPORT["widths"] += 2
                REPORT["width0"] += int(b[1] == b[0]) + int(b[3] == b[2])
                REPORT["wmax"] = max(REPORT["wmax"], b[1] - b[0], b[3] - b[2])
            REPORT["rows"] += 1
    REPORT["pairs"] += pairs
    REPORT["excused"] += excused
    return pairs, excused


def _cohort(edlib, setting):
    """the posterior test's cohort, 130 samples, run once per setting: the device's likelihood matrix, the batch's call table and its
    bounds (batch route), the checker's chains, the pseudo-rows (one per maximal run of gamma(T) > 1/2) and their bounds (plan route)"""
    key = ("cohort", setting)
    if key not in _CACHE:
        L = _layout()
        plan, trs = _plan(edlib, L, setting)
        b = edlib.Batch(plan, S_MAX)
        test, ref, phi, p = _counts()
        b.run(test, ref, phi, p)
        ll, calls, dlp = b.loglik(), b.calls(), b.posterior(log=True)
        got = {lv: b.call_bounds(lv) for lv in NEST}
        assert b.n_posterior_passes() == 1
        b.close()
        want = pc.run(ll, L.chrom_off, trs, np.longdouble)
        sp = []
        for c, res in enumerate(want):
            if res is None:
                continue
            lo = int(L.chrom_off[c])
            sp += [(s, c, r0, r1, t) for s in range(S_MAX) for t in (1, 2) for r0, r1 in bc.pseudo_rows(res, t, s, lo)]
        pseudo = _rows(*(np.array(x) for x in zip(*sp)))
        post = plan.posterior(ll, S_MAX)
        assert post.log_posterior().tobytes() == dlp.tobytes()          # both routes walk the same log gamma
        got_pseudo = {lv: post.call_bounds(pseudo, lv) for lv in NEST}
        got_plan = {lv: post.call_bounds(calls, lv) for lv in LEVELS}
        post.free()
        plan.close()
        _CACHE[key] = types.SimpleNamespace(L=L, trs=trs, ll=ll, dlp=dlp, calls=calls, got=got, want=want, pseudo=pseudo, got_pseudo=got_pseudo,
                                            got_plan=got_plan)
    return _CACHE[key]


@pytest.mark.parametrize("setting", [1, LOUD])
def test_the_posterior_cohort_against_the_checker(edlib, setting):
    """chains of 1 .. 513 exons with an empty chromosome among them, 130 samples: the batch's own call table and the pseudo-rows"""
    k = _cohort(edlib, setting)
    assert len(k.calls) > 1000 and len(k.pseudo) > 1000
    assert set(np.unique(k.calls["type"])) <= {1, 2}
    for rows, got in ((k.calls, k.got), (k.pseudo, k.got_pseudo)):
        pairs, excused = _verify(k.L, k.trs, k.want, k.ll, k.dlp, rows, got)
        assert pairs > 8000 and excused <= 0.01 * pairs, (pairs, excused)


def _wall_case(t):
    """one chain of 513 exons (and chains of 1, 2, 64, 65), starts 500 bp apart; the column of type t is 12.0 and the other two 0; sample
    i has walls of -60.0 in t's column at exons 256 -+ (D[i] + 1), the last sample none.  Rows [256, 256] of type t for every sample, and
    rows on the first and the last exon of every short chain."""
    D = (1, 2, 63, 64, 65, 127, 128, 129, 200)
    sizes = (513, 1, 2, 64, 65)
    L = types.SimpleNamespace(sizes=list(sizes), chrom_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), E=sum(sizes), C=len(sizes))
    L.start = (1000 + 500 * np.arange(L.E)).astype(np.int32)
    L.end = (L.start + 120).astype(np.int32)
    S = len(D) + 1
    ll = np.zeros((L.E, 3, S))
    col = pc.COL[t]
    ll[:, col, :] = 12.0
    for i, d in enumerate(D):
        ll[256 - (d + 1), col, i] = ll[256 + (d + 1), col, i] = -60.0
    want_b = [(256 - d, 256 + d) for d in D] + [(0, 512)]
    rows = [(s, 0, 256, 256, t) for s in range(S)]
    for c in range(1, L.C):
        lo, hi = int(L.chrom_off[c]), int(L.chrom_off[c + 1])
        rows += [(s, c, x, x, t) for s in (0, S - 1) for x in sorted({lo, hi - 1})]
    return L, D, ll, want_b, _rows(*(np.array(x) for x in zip(*rows)))


def _wall_condition(t):
    """on the CPU, with the checker's arithmetic, before any device value is read: all four bounds of sample i sit exactly at
    256 -+ D[i], far from both thresholds -- inside the walls G is between -2e-4 and 0 against log 0.975 = -0.0253, at a wall below -50
    against log 0.025 = -3.69; without walls the bounds are the chain's ends"""
    key = ("wall", t)
    if key not in _CACHE:
        L, D, ll, want_b, rows = _wall_case(t)
        tp, ln = SETTINGS[1]
        trs = pc.transitions(L.chrom_off, L.start, L.end, tp, ln)
        want = pc.run(ll, L.chrom_off, trs, np.longdouble)
        for s, (b0, b1) in enumerate(want_b):
            rec = bc.row(want[0], ll[:513], trs[0], 256, 256, t, s, LEVELS)
            for lv in LEVELS:
                assert rec["bounds"][lv] == (b0, b0, b1, b1), (t, s, lv, rec["bounds"][lv])
            GL, GR = rec["ext"]["GL"].astype(np.float64), rec["ext"]["GR"].astype(np.float64)
            assert np.all(GL[:256 - b0 + 1] > -2e-4) and np.all(GR[:b1 - 256 + 1] > -2e-4)
            if s < len(D):
                assert GL[256 - b0 + 1] < -50 and GR[b1 - 256 + 1] < -50
        _CACHE[key] = (L, trs, want, ll, want_b, rows)
    return _CACHE[key]


@pytest.mark.parametrize("t", [1, 2])
def test_tile_edges(edlib, t):
    """walks that end one exon before, on and after the edge of the first and the second tile of 64, and in the fourth; walks that reach
    the chain's ends after 256 steps; chains of 1, 2, 64 and 65 exons"""
    L, trs, want, ll, want_b, rows = _wall_condition(t)
    plan, _ = _plan(edlib, L, 1)
    post = plan.posterior(ll, ll.shape[2])
    got = {lv: post.call_bounds(rows, lv) for lv in LEVELS}
    dlp = post.log_posterior()
    post.free()
    plan.close()
    for lv in LEVELS:
        for s, (b0, b1) in enumerate(want_b):
            q = got[lv][s]
            assert (q["anchor_exon"], q["start_lo"], q["start_hi"], q["end_lo"], q["end_hi"], q["flags"]) == (256, b0, b0, b1, b1, 0), (lv, s, q)
            assert q["log_keep_start"] == 0.0 and q["log_keep_end"] == 0.0
    pairs, excused = _verify(L, trs, want, ll, dlp, rows, got)
    assert excused == 0 and pairs == 8 * len(rows)


def test_flagged_rows_and_impossible_exons(edlib):
    """a row whose column is -inf over the whole row and rows of type 0 are flagged and keep their own indices; a row that only reaches
    into the -inf block is walked, and its log_keep_end is -inf"""
    L = Layout((40, 70), 5)
    S = 3
    rng = np.random.default_rng(17)
    ll = -rng.gamma(2.0, 3.0, (L.E, 3, S))
    ll[10:20, 0, 1] = -np.inf                        # sample 1: deletion impossible at exons 10 .. 19
    ll[50:60, 0, 1] += 25.0                          # ... and loud at 50 .. 59 (chain 1: exons 40 .. 109)
    ll[45:50, 2, 2] = -np.inf                        # sample 2: duplication impossible at 45 .. 49, loud next to it
    ll[50:56, 2, 2] += 25.0
    plan, trs = _plan(edlib, L, 1)
    want = pc.run(ll, L.chrom_off, trs, np.longdouble)
    rows = _rows(*(np.array(x) for x in zip(*[
        (1, 0, 10, 19, 1), (1, 0, 12, 12, 1),        # -inf over the whole row
        (1, 0, 5, 19, 1), (1, 0, 10, 30, 1),         # reach into the block from either side
        (1, 1, 50, 59, 1), (2, 1, 50, 55, 2), (2, 1, 45, 55, 2), (2, 1, 50, 109, 2),
        (0, 0, 3, 9, 0), (1, 1, 50, 59, 0), (2, 1, 40, 109, 3)])))
    post = plan.posterior(ll, S)
    got = {lv: post.call_bounds(rows, lv) for lv in LEVELS}
    dlp = post.log_posterior()
    post.free()
    plan.close()
    for lv in LEVELS:
        for n in (0, 1, 8, 9, 10):
            _check_flagged(rows[n], got[lv][n])
        assert np.all(got[lv]["flags"][2:8] == 0)
        assert np.isneginf(got[lv]["log_keep_end"][2]) and np.isneginf(got[lv]["log_keep_start"][3]) and np.isneginf(got[lv]["log_keep_start"][6])
        assert got[lv]["end_hi"][2] <= 9 and got[lv]["start_lo"][3] >= 20 and got[lv]["start_lo"][6] >= 50
    before = REPORT["flagged"]
    _verify(L, trs, want, ll, dlp, rows, got)
    assert REPORT["flagged"] - before == 5 * len(LEVELS)


def test_anchor_rule_on_planted_ties(edlib):
    """exact ties and NaN written into the device's log gamma itself: the anchor is the lowest exon among equal maxima -- in one lane's
    successive tiles, in neighbouring lanes, with the lower exon in lane 63 and the higher in lane 0 of the next tile, three tiles apart --
    NaN is ignored wherever it stands, -0.0 ties with 0.0, and a row of NaN and -inf only is flagged"""
    from exomedepth_amd._lib import check, lib
    L = Layout((300, 7), 23)
    S = 8
    ll = -np.random.default_rng(29).gamma(2.0, 3.0, (L.E, 3, S))
    plan, _ = _plan(edlib, L, 1)
    post = plan.posterior(ll, S)
    lp = np.minimum(post.log_posterior(), -1.0)                    # every value below the planted maximum
    r0, r1, top = 10, 250, -0.25
    plants = [((60, 124, 125, 190), ()),                           # offsets from r0: tile 0 lane 60, tile 1 lanes 60 and 61, tile 2 lane 62
              ((63, 64), ()),                                      # lane 63 of tile 0 against lane 0 of tile 1
              ((64, 127, 128), (0, 1, 63)),                        # NaN in front, first maximum in lane 0 of tile 1
              ((239, 240), (238,)),                                # the row's last two exons, a NaN before them
              ((5, 6), (5,)),                                      # a NaN ON the first of two maxima: the second is the anchor
              ((0, 240), ()),                                      # the row's two ends
              ((100,), tuple(range(0, 100)) + tuple(range(101, 241))),   # everything else NaN
              ((), tuple(range(0, 241, 2)))]                       # NaN and -inf only: flagged
    want_off = [60, 63, 64, 239, 6, 0, 100, None]
    rows = []
    for s, (tie, nan) in enumerate(plants):
        t = 1 + s % 2
        if not tie:
            lp[r0:r1 + 1, t - 1, s] = -np.inf
        lp[r0 + np.array(tie, dtype=np.int64), t - 1, s] = top
        lp[r0 + np.array(nan, dtype=np.int64), t - 1, s] = np.nan
        rows.append((s, 0, r0, r1, t))
    lp[r0 + 0, 1, 5], lp[r0 + 240, 1, 5] = -0.0, 0.0               # sample 5 (type 2): the zeros of both signs, the lower exon first
    rows += [(0, 1, 300, 306, 1)]                                  # an untouched short chain beside them
    rows = _rows(*(np.array(x) for x in zip(*rows)))
    check(lib().ed_memcpy_h2d(post.device_pointers()["logpost"], lp.ctypes.data, lp.nbytes))
    assert post.log_posterior().tobytes() == lp.tobytes()
    got = post.call_bounds(rows, 0.95)
    post.free()
    plan.close()
    for n, off in enumerate(want_off):
        da = _device_anchor(lp, rows[n])
        assert (da is None) == (off is None) and (off is None or da[0] == r0 + off), (n, da)        # the rule as this file states it
        _check_anchor(rows[n], got[n], da)
        if off is not None:
            assert got[n]["start_lo"] <= got[n]["start_hi"] <= r0 + off <= got[n]["end_lo"] <= got[n]["end_hi"]
    _check_anchor(rows[-1], got[-1], _device_anchor(lp, rows[-1]))


def test_a_row_depends_on_the_row_alone(edlib):
    """bit for bit the same record at batch widths 1 .. 130 and with the rows in shuffled order, for every row; and for a row alone, for a
    sample of 200 rows: the 60 longest, 70 of the 513-exon chain (the longest walks) and 70 drawn at random"""
    k = _cohort(edlib, 1)
    L = k.L
    rows = np.concatenate([k.calls, k.pseudo])
    ref = np.concatenate([k.got[0.95], k.got_pseudo[0.95]])
    plan, _ = _plan(edlib, L, 1)
    for S in WIDTHS:
        sel = np.flatnonzero(rows["sample"] < S)
        post = plan.posterior(np.ascontiguousarray(k.ll[:, :, :S]), S)
        assert post.call_bounds(rows[sel], 0.95).tobytes() == ref[sel].tobytes(), S
        post.free()
    post = plan.posterior(k.ll, S_MAX)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(rows))
    assert post.call_bounds(rows[perm], 0.95).tobytes() == ref[perm].tobytes()
    longest = np.argsort(-rows["nexons"], kind="stable")[:60]
    reach = (ref["end_hi"] - ref["start_lo"]).astype(np.int64)
    big = np.flatnonzero(rows["chrom"] == L.sizes.index(513))
    big = big[np.argsort(-reach[big], kind="stable")[:70]]
    alone = np.unique(np.concatenate([longest, big, perm[:70]]))
    assert rows["nexons"][alone].max() == rows["nexons"].max() and reach[alone].max() == reach[big].max()
    for n in alone:
        assert post.call_bounds(rows[n:n + 1], 0.95).tobytes() == ref[n:n + 1].tobytes(), n
    post.free()
    plan.close()


def test_levels_nest(edlib):
    """the intervals at 0.5, 0.8, 0.95 and 0.999 lie inside one another, row by row; anchor and the three doubles do not depend on the level"""
    for setting in (1, LOUD):
        k = _cohort(edlib, setting)
        for got in (k.got, k.got_pseudo):
            for inner, outer in zip(NEST[:-1], NEST[1:]):
                gi, go = got[inner], got[outer]
                assert np.all(go["start_lo"] <= gi["start_lo"]) and np.all(gi["start_hi"] <= go["start_hi"])
                assert np.all(go["end_lo"] <= gi["end_lo"]) and np.all(gi["end_hi"] <= go["end_hi"])
                for name in ("anchor_exon", "flags") + DOUBLES:
                    assert gi[name].tobytes() == go[name].tobytes(), name
            assert np.any(got[0.999]["start_lo"] < got[0.5]["start_lo"]) and np.any(got[0.999]["start_hi"] > got[0.5]["start_hi"])


def test_batch_route_and_plan_route(edlib):
    k = _cohort(edlib, 1)
    for lv in LEVELS:                                   # the batch route equals the plan route bit for bit
        assert k.got[lv].tobytes() == k.got_plan[lv].tobytes()
    L = _layout()
    S = 17
    dA, dB = ([np.ascontiguousarray(x[..., :S]) for x in _counts(seed)] for seed in (7, 8))
    plan, _ = _plan(edlib, L, 1)
    b = edlib.Batch(plan, S)
    b.enable_timing()
    b.run(*dA)
    assert b.call_bounds_ms() == 0.0
    first = b.call_bounds()
    assert first.dtype == CALL_BOUNDS_DTYPE and len(first) == b.n_calls() > 0
    assert b.call_bounds_ms() > 0.0
    sel = np.flatnonzero(k.calls["sample"] < S)         # (a sample does not depend on the batch width)
    assert first.tobytes() == k.got[0.95][sel].tobytes()
    assert b.call_bounds(0.5).tobytes() == k.got[0.5][sel].tobytes() and b.call_bounds(0.95).tobytes() == first.tobytes()
    b.call_posterior()
    assert b.n_posterior_passes() == 1                  # a second request, at another level too, launches only the kernel
    b.run(*dB)                                          # a new run invalidates the result
    assert b.call_bounds_ms() == 0.0
    second = b.call_bounds()
    assert b.n_posterior_passes() == 2 and len(second) == b.n_calls()
    fresh = edlib.Batch(plan, S)
    fresh.run(*dB)
    assert second.tobytes() == fresh.call_bounds().tobytes() and second.tobytes() != first.tobytes()
    fresh.close()
    for bad in (0.0, 1.0, -0.1, float("nan")):          # refused before anything is enqueued
        with pytest.raises(edlib.EdError, match="level"):
            b.call_bounds(bad)
    assert b.n_posterior_passes() == 2
    post = plan.posterior(b.loglik(), S)
    calls = b.calls()
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(edlib.EdError, match="level"):
            post.call_bounds(calls, bad)
    outside = calls[:1].copy()
    outside["end_exon"] = L.chrom_off[int(outside["chrom"][0]) + 1]
    with pytest.raises(edlib.EdError, match="inside its chromosome"):
        post.call_bounds(outside)
    assert post.call_bounds(calls[:0]).size == 0
    post.free()
    b.close()
    f = edlib.Batch(plan, S)                            # fused mode without the matrix: the posterior's own error
    f.set_fused(True)
    f.keep_loglik(False)
    f.run(*dA)
    with pytest.raises(edlib.EdError, match="likelihood matrix"):
        f.call_bounds()
    f.close()
    co = edlib.Cohort(plan, S, 2)                       # Cohort.results
    dev = [edlib.DeviceArray(x) for x in dA]
    t = co.submit(dev[0], dev[1], dev[2], dev[3], n_samples=S)
    assert "call_bounds" not in co.results(t, S) and "call_bounds" not in co.results(t, S, posterior=True)
    out = co.results(t, S, breakpoints=0.95)
    assert out["call_bounds"].tobytes() == first.tobytes() and "call_posterior" not in out
    co.close()
    plan.close()


def test_callcnvs_columns(edlib):
    L = _layout()
    test, ref, phi, p = _counts()
    tp, ln = SETTINGS[1]
    rows = np.concatenate([np.arange(L.chrom_off[c], L.chrom_off[c + 1]) for c in (L.sizes.index(257), L.sizes.index(513))])
    chrom = np.repeat(["1", "2"], [257, 513])
    names = np.array(["e%d" % i for i in range(rows.size)], dtype=object)
    ct, cr = test[rows, 0].astype(float), ref[rows, 0].astype(float)
    st_, en_ = L.start[rows], (L.start[rows] + 60).astype(np.int32)
    base = ("start.p", "end.p", "type", "nexons", "start", "end", "chromosome", "id", "BF", "reads.expected", "reads.observed", "reads.ratio")
    post4 = ("post.mean", "post.min", "post.all", "log.evidence")
    ten = ("start.p.lo", "start.p.hi", "end.p.lo", "end.p.hi", "start.lo", "start.hi", "end.lo", "end.hi", "start.keep", "end.keep")
    for phi_x in (float(phi[0]), np.where(np.arange(rows.size) % 2 == 0, phi[0], 1.5 * phi[0])):
        x = edlib.ExomeDepth(ct, cr, phi=phi_x, expected=float(p[0]))
        x.CallCNVs(chrom, st_, en_, names, tp, ln)
        quiet = [dict(r) for r in x.CNV_calls]
        assert quiet and all(tuple(r.keys()) == base for r in quiet)
        x.CallCNVs(chrom, st_, en_, names, tp, ln, posterior=True)
        assert all(tuple(r.keys()) == base + post4 for r in x.CNV_calls)
        with_post = [dict(r) for r in x.CNV_calls]
        x.CallCNVs(chrom, st_, en_, names, tp, ln, posterior=True, breakpoints=True)
        assert all(tuple(r.keys()) == base + post4 + ten for r in x.CNV_calls)
        assert [{k: r[k] for k in base + post4} for r in x.CNV_calls] == with_post
        both = [dict(r) for r in x.CNV_calls]
        x.CallCNVs(chrom, st_, en_, names, tp, ln, breakpoints=0.95)
        assert all(tuple(r.keys()) == base + ten for r in x.CNV_calls)
        assert [{k: r[k] for k in base} for r in x.CNV_calls] == quiet
        assert [{k: r[k] for k in ten} for r in x.CNV_calls] == [{k: r[k] for k in ten} for r in both]
        wide = [dict(r) for r in x.CNV_calls]
        x.CallCNVs(chrom, st_, en_, names, tp, ln, breakpoints=0.5)
        # the plan route on the same slot gives the same numbers
        pl = edlib.Plan(np.array([0, 257, 770], np.int32), st_, en_, tp, ln)
        po = pl.posterior(np.ascontiguousarray(x.likelihood).reshape(-1, 3, 1), 1)
        tab = np.zeros(len(quiet), dtype=CALL_DTYPE)
        tab["chrom"] = [int(r["chromosome"]) - 1 for r in quiet]
        tab["start_exon"] = [r["start.p"] - 1 for r in quiet]
        tab["end_exon"] = [r["end.p"] - 1 for r in quiet]
        tab["type"] = [1 if r["type"] == "deletion" else 2 for r in quiet]
        cb = po.call_bounds(tab, 0.95)
        po.free()
        pl.close()
        for r, w, q in zip(x.CNV_calls, wide, cb):
            assert (w["start.p.lo"], w["start.p.hi"], w["end.p.lo"], w["end.p.hi"]) == tuple(int(q[k]) + 1 for k in BOUNDS)
            assert (w["start.keep"], w["end.keep"]) == (float(np.exp(q["log_keep_start"])), float(np.exp(q["log_keep_end"])))
            for d in (r, w):
                assert 1 <= d["start.p.lo"] <= d["start.p.hi"] <= d["end.p.lo"] <= d["end.p.hi"] <= rows.size
                assert (d["start.lo"], d["start.hi"]) == (int(st_[d["start.p.lo"] - 1]), int(st_[d["start.p.hi"] - 1]))
                assert (d["end.lo"], d["end.hi"]) == (int(en_[d["end.p.lo"] - 1]), int(en_[d["end.p.hi"] - 1]))
                assert 0.0 <= d["start.keep"] <= 1.0 + 1e-12 and 0.0 <= d["end.keep"] <= 1.0 + 1e-12
            assert w["start.p.lo"] <= r["start.p.lo"] and r["start.p.hi"] <= w["start.p.hi"]       # 0.5 inside 0.95
            assert w["end.p.lo"] <= r["end.p.lo"] and r["end.p.hi"] <= w["end.p.hi"]


def test_report():
    """the figures quoted in DESIGN.md 4.20 (printed with -s); the fraction is of the bar of this file's docstring"""
    print("\nbounds: %(rows)d rows checked, %(pairs)d (row, bound) pairs, %(excused)d excused near a threshold, %(ties)d rows whose anchor is not the "
          "long-double arg-max, %(flagged)d flagged records; largest deviation of a double as a fraction of its bar %(frac).4f; longest walk %(longest)d "
          "steps; %(width0)d of %(widths)d intervals of width 0, widest %(wmax)d exons" % REPORT)
    assert REPORT["rows"] > 0 and REPORT["pairs"] > 0
