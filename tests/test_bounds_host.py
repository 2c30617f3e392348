"""Breakpoint credible intervals without a device: the checker (tests/bounds_checker.py) against a sum over all paths, the C-ABI and the
Python names of the feature, and the condition under which the GPU test may excuse an index: threshold decisions that lie within the
numerical bar are rare (at most 1 % of the (row, bound) pairs), asserted here on CPU-made likelihoods with the checker alone."""
import itertools
import os
import re

import numpy as np

import bounds_checker as bc
import posterior_checker as pc
from test_gpu_chain_geometry import LOUD, SETTINGS
from test_gpu_posterior import _counts, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.5, 0.95)


def _brute(ll, tr):
    """log joint probability of every path of a chain (m, 3) with its data, the closing step included: dict path -> log p"""
    m = ll.shape[0]
    out = {}
    with np.errstate(invalid="ignore"):
        for path in itertools.product(range(3), repeat=m):
            lp, prev = 0.0, 0
            for i, x in enumerate(path):
                lp += float(pc._lt(tr, i, np.float64)[prev, x]) + float(ll[i, pc.COL[x]])
                prev = x
            out[path] = lp + float(pc._lt(tr, m, np.float64)[prev, 0])
    return out


def _lse(v):
    v = np.asarray(v, dtype=np.float64)
    mx = v.max() if v.size else -np.inf
    return -np.inf if not np.isfinite(mx) else float(mx + np.log(np.sum(np.exp(v - mx))))


def test_extent_equals_the_sum_over_all_paths():
    """G_L and G_R of the checker against brute force for m <= 7: every anchor, both types, a gap of 0 (C = -inf) in the chain"""
    rng = np.random.default_rng(3)
    n = 0
    for m in (1, 2, 3, 5, 7):
        gaps = rng.integers(100, 4000, m)
        if m >= 3:
            gaps[2] = 0
        start = (1000 + np.cumsum(gaps)).astype(np.int32)
        end = (start + 80).astype(np.int32)
        off = np.array([0, m], np.int32)
        for tp, ln in (SETTINGS[1], SETTINGS[LOUD]):
            tr = pc.transitions(off, start, end, tp, ln)[0]
            assert m < 3 or np.isneginf(tr["C"][2])
            ll = -rng.gamma(2.0, 2.0, (m, 3, 1))
            res = pc.chain(ll, tr, np.longdouble)
            paths = _brute(ll[:, :, 0], tr)
            lz = _lse(list(paths.values()))
            assert abs(lz - float(res["logZ"][0])) < 1e-10
            for t in (1, 2):
                for a in range(m):
                    ext = bc.extent(res, ll, tr, a, t, 0)
                    lga = _lse([v for p, v in paths.items() if p[a] == t]) - lz
                    assert abs(lga - float(res["log_gamma"][a, t, 0])) < 1e-10
                    for i in range(a + 1):
                        want = _lse([v for p, v in paths.items() if all(x == t for x in p[i:a + 1])]) - lz - lga
                        assert abs(float(ext["GL"][a - i]) - want) < 1e-9, (m, t, a, i)
                    for j in range(a, m):
                        want = _lse([v for p, v in paths.items() if all(x == t for x in p[a:j + 1])]) - lz - lga
                        assert abs(float(ext["GR"][j - a]) - want) < 1e-9, (m, t, a, j)
                        n += 1
                    # in exact arithmetic G does not increase outward
                    assert np.all(np.diff(ext["GL"].astype(np.float64)) <= 1e-12) and np.all(np.diff(ext["GR"].astype(np.float64)) <= 1e-12)
    assert n > 100


def test_first_failure_and_anchor_rules():
    G = np.array([0.0, -0.01, -0.5, -0.02, -9.0], dtype=np.longdouble)            # not monotone: the walk stops at the first failure
    assert bc.first_failure(G, -0.1) == 1 and bc.first_failure(G, -1.0) == 3 and bc.first_failure(G, -10.0) == 4
    assert bc.first_failure(np.array([0.0, np.nan, 0.0], dtype=np.longdouble), -5.0) == 0
    lg = np.full((6, 3, 1), -1.0, dtype=np.longdouble)
    lg[:, 1, 0] = [np.nan, -0.3, -0.1, -0.1, -0.2, np.nan]
    res = {"log_gamma": lg}
    assert bc.anchor(res, 0, 5, 1, 0) == (2, lg[2, 1, 0])                         # ties to the lowest index, NaN ignored
    assert bc.anchor(res, 3, 5, 1, 0)[0] == 3 and bc.anchor(res, 5, 5, 1, 0) == (None, None)
    lg[:, 2, 0] = -np.inf
    assert bc.anchor(res, 0, 5, 2, 0) == (None, None)
    thi, tlo = bc.thresholds(0.95)
    assert abs(thi - np.log(0.975)) < 1e-15 and abs(tlo - np.log(0.025)) < 1e-15


def test_entries_are_declared_and_bound():
    """fails without the feature: the three entries in the header and in _lib.SYMBOLS, the record of 48 bytes, the Python names"""
    import exomedepth_amd
    from exomedepth_amd import _lib, api
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("ed_plan_call_bounds", "ed_batch_copy_call_bounds", "ed_batch_call_bounds_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and name in bound, name
    assert re.search(r"typedef struct \{[^}]*anchor_exon[^}]*log_keep_end[^}]*\}\s*ed_call_bounds;", text)
    assert api.CALL_BOUNDS_DTYPE.itemsize == 48 and exomedepth_amd.CALL_BOUNDS_DTYPE is api.CALL_BOUNDS_DTYPE
    assert api.CALL_BOUNDS_DTYPE.names == ("anchor_exon", "start_lo", "start_hi", "end_lo", "end_hi", "flags", "log_anchor", "log_keep_start",
                                           "log_keep_end")
    assert [api.CALL_BOUNDS_DTYPE.fields[k][1] for k in api.CALL_BOUNDS_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert api.CALL_POST_DTYPE.itemsize == 32                                     # ed_call_post is not extended
    for cls, name in ((api.Posterior, "call_bounds"), (api.Batch, "call_bounds"), (api.Batch, "call_bounds_ms")):
        assert callable(getattr(cls, name))
    src = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    assert '#include "edbounds.inc"' in src


def test_threshold_decisions_near_the_bar_are_rare(oracle):
    """the condition behind the GPU test's excuse, with the checker alone: likelihoods of the posterior test's counts made on the CPU,
    12 samples, SETTINGS[1] and LOUD, levels 0.5 and 0.95, one row per maximal run of gamma(T) > 1/2"""
    L = _layout()
    test, ref, phi, p = _counts()
    S = 12
    cols = []
    for s in range(S):
        ll, nerr = oracle.get_loglike_matrix(phi[s], p[s], test[:, s] + ref[:, s], test[:, s], 1.0, oracle.PORTABLE)
        assert nerr == 0
        cols.append(np.asarray(ll))
    ll = np.ascontiguousarray(np.stack(cols, axis=2))
    decisions = near = rows = 0
    widths = []
    longest = 0
    for setting in (1, LOUD):
        tp, ln = SETTINGS[setting]
        trs = pc.transitions(L.chrom_off, L.start, L.end, tp, ln)
        want = pc.run(ll, L.chrom_off, trs, np.longdouble)
        for c, res in enumerate(want):
            if res is None:
                continue
            lo, m = int(L.chrom_off[c]), L.sizes[c]
            specs = [(r0, r1, t, s) for s in range(S) for t in (1, 2) for r0, r1 in bc.pseudo_rows(res, t, s)]
            recs = bc.rows(res, ll[lo:lo + m], trs[c], specs, LEVELS, window=8)       # (a small window: some rows take the row-by-row way)
            for n, ((r0, r1, t, s), rec) in enumerate(zip(specs, recs)):
                assert rec is not None
                rows += 1
                if n % 7 == 0:                                                        # the two ways of the checker agree
                    one = bc.row(res, ll[lo:lo + m], trs[c], r0, r1, t, s, LEVELS)
                    assert one["bounds"] == rec["bounds"] and one["anchor"] == rec["anchor"]
                    assert all(one[k] == rec[k] for k in ("log_anchor", "log_keep_start", "log_keep_end", "bar_keep_start", "bar_keep_end"))
                for level in LEVELS:
                    b = rec["bounds"][level]
                    assert 0 <= b[0] <= b[1] <= rec["anchor"] <= b[2] <= b[3] < m
                    assert r0 <= rec["anchor"] <= r1
                    decisions += 4
                    near += bc.near_threshold(rec, level)
                    widths += [b[1] - b[0], b[3] - b[2]]
                    longest = max(longest, rec["anchor"] - b[0], b[3] - rec["anchor"])
    print("\nbounds (checker alone): %d rows, %d threshold decisions, %d within the bar; widths 0: %.0f %%, max %d; longest walk %d steps"
          % (rows, decisions, near, 100.0 * np.mean(np.array(widths) == 0), max(widths), longest))
    assert rows > 1000 and near <= 0.01 * decisions
    assert 0 in widths and max(widths) >= 3          # the intervals are not all trivial
