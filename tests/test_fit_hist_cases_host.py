"""tests/fit_hist_cases.py is what tests/test_gpu_fit_edges.py takes it for -- checked without a GPU and without the library:
the restated constants are the source's, the catalogue reaches every route, edge, walk, width and capacity it names (asserted on the
restatement), and every column held to the checker is well conditioned AND sensitive: the checker's own MLE moves by more than 1000 x the
GPU test's bar when the planted cells move by one count, when one cell is lost and when a run of rows is counted twice."""
import os
import re

import numpy as np
import pytest

import fit_hist_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_REL_TOL = 1e-8           # tests/test_gpu_fit_invariance.py (a GPU module: restated, test_gpu_fit_edges.py imports the original)
HOT_BARS = (1e-6, 1e-8)      # tests/test_gpu_fit.py::test_sample_major_histograms_with_bins_that_leave_the_lds_early: phi, expected
NM_BARS = (2e-3, 2e-4)       # tests/test_gpu_fit_concordance.py: fit mode 1 against oracle.fit_nm, phi and p
SENSITIVE = 1000.0
PHI_MIN = 3e-3


def _src(name):
    with open(os.path.join(ROOT, "exomedepth_amd", "csrc", name)) as f:
        return f.read()


# ---- the constants are the source's -------------------------------------------------------------------------------------------------------

def test_constants_match_the_source():
    hist, job, fit = _src("edfit_hist.inc"), _src("ed_fit_job.hpp"), _src("edfit.inc")

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    assert sorted(int(v) for v in re.findall(r"#define ED_HG_KS (\d+)", fit)) == sorted(fc.GEOMETRIES)
    one(hist, r"constexpr int kHistId = ED_HG_KS;")
    one(hist, r"constexpr int kHistSamples = kHistId;")
    ky = int(one(hist, r"constexpr int kHistKy = (\d+) \* 8 / kHistId;"))
    kr = int(one(hist, r"constexpr int kHistKr = (\d+) \* 8 / kHistId;"))
    kn = int(one(hist, r"constexpr int kHistKn = (\d+) \* 8 / kHistId;"))
    k2_2, k2 = (int(v) for v in one(hist, r"constexpr int kOv2 = \(kHistId == 2\) \? (\d+) : (\d+);"))
    one(hist, r"constexpr int kOv2R0 = kHistKr - kHistKy;")
    one(hist, r"constexpr int kHistK = kHistKy \+ kHistKr \+ kHistKn;")
    one(hist, r"constexpr bool kSm2 = \(kHistId != 2\);")
    one(hist, r"constexpr int kSmBins = kHistK \+ \(kSm2 \? 2 \* kOv2 : 0\);")
    block = int(one(hist, r"constexpr int kHistBlock = (\d+);"))
    halves = int(one(hist, r"constexpr int kHistHalves = (\d+);"))
    one(hist, r"constexpr int kHistRows = kHistBlock / kHistSamples;")
    one(hist, r"constexpr int kHistGroups = kHistHalves \* kHistRows;")
    for g in fc.GEOMETRIES:
        G = fc.GEO[g]
        assert (G.Ky, G.Kr, G.Kn) == (ky * 8 // g, kr * 8 // g, kn * 8 // g)
        assert G.K2 == (k2_2 if g == 2 else k2) and G.R0 == G.Kr - G.Ky
        assert G.rows == block // g and G.G == halves * G.rows
        assert G.sm_bins == G.Ky + G.Kr + G.Kn + (0 if g == 2 else 2 * G.K2)
    assert (fc.HIST_BLOCK, fc.HIST_HALVES) == (block, halves)
    assert fc.HIST_CHUNK == int(one(hist, r"constexpr int kHistChunk = (\d+);"))
    a, b = (int(v) for v in one(hist, r"constexpr int kSmChunk = (\d+) - (\d+);"))
    assert fc.SM_CHUNK == a - b == 48128
    assert fc.SM_HOT == int(one(hist, r"constexpr uint32_t kSmHot = (0x[0-9a-fA-F]+);"), 16) == 16384
    assert fc.SM_CARRY == int(one(hist, r"constexpr int kSmCarry = (\d+);"))
    assert fc.HS_BLOCK == int(one(hist, r"constexpr int kHsBlock = (\d+);"))
    assert fc.HN_S == int(one(hist, r"constexpr int kHnS = (\d+);"))
    spans = sorted(int(v) for v in re.findall(r"constexpr int64_t kSpan = \(int64_t\)kHsBlock \* (\d+);", hist))
    assert spans == [4, 8] and (fc.SPAN32, fc.SPAN16) == (fc.HS_BLOCK * 4, fc.HS_BLOCK * 8) == (1024, 2048)
    # the halves, the chunk walk and the list a row lands on
    one(hist, r"const int64_t r0 = \(E \* half\) / kHistHalves, r1 = \(E \* \(half \+ 1\)\) / kHistHalves;")
    one(hist, r"const int region = half \* kHistRows \+ tid / kHistSamples;")
    one(hist, r"const int64_t e0 = c0 \+ tid / kHistSamples;")
    one(hist, r"const int64_t per = \(nwg \+ 7\) / 8;|nwg = ng \* kHistHalves, per = \(nwg \+ 7\) / 8;")
    # the lists' capacity
    lim, lo, div = (int(v) for v in one(hist, r"cap_of\(int64_t E\) \{ return std::min<int64_t>\((\d+) / kHistGroups, std::max<int64_t>\((\d+), "
                                              r"\(E / kHistGroups\) / (\d+) \+ 1\)\); \}"))
    for g in fc.GEOMETRIES:
        for E in (1, 2597, 10277, 262143, 1060865, 10 ** 7):
            assert fc.cap(E, g) == min(lim // fc.GEO[g].G, max(lo, (E // fc.GEO[g].G) // div + 1))
    # the automatic geometry and the rows its depth is taken from
    d8, d4 = (int(v) for v in one(job, r"fit_hist_geometry\(int depth\) \{ return depth <= (\d+) \? 8 : \(depth <= (\d+) \? 4 : 2\); \}"))
    assert (fc.DEPTH_8, fc.DEPTH_4) == (d8, d4)
    one(fit, r"const int mstride = j\.mode == 1 \? 1 : \(E >= 65536 \? 16 : 4\);")
    assert len(re.findall(r"atomicMax\(depth_max, \(int\)fmin\(t?sn / t?cnt, 2\.0e9\)\);", fit)) == 2


# ---- coverage, on the restatement ---------------------------------------------------------------------------------------------------------

def _planted_routes(case, s):
    c = case.cols[s]
    return fc.route(c.y[c.planted], c.r[c.planted], case.geometry, case.layout)


def test_group_A_reaches_every_route_at_every_edge():
    seen = {}
    for case in fc.group_A():
        g, G = case.g, fc.GEO[case.g]
        col = case.cols[case.slot]
        edge = [e for e in fc.edge_values(g) if e[0] == col.name][0]
        y, r = col.y[col.planted].astype(np.int64), col.r[col.planted].astype(np.int64)
        on_edge = {"n": y + r, "r": r, "y": y, "zero": y + r}[edge[1]] == edge[2]
        assert on_edge.all() and len(col.planted) >= int(0.09 * fc.E_A), case.name
        routes = _planted_routes(case, case.slot)
        seen.setdefault((g, case.layout), set()).update(int(v) for v in routes)
        dominant = int(np.argmax(np.bincount(routes, minlength=5)))
        seen[(g, case.layout, edge[0])] = dominant
        assert not any(case.ran_out(s) for s in range(case.S) if s != case.slot), case.name
        assert (case.S, case.slot, case.E) == (5, 2, 2048)
    for g in fc.GEOMETRIES:
        for layout in (0, 1):
            want = {fc.SKIP, fc.FIRST, fc.SECOND, fc.LIST} | ({fc.MIXED} if layout == 1 and g != 2 else set())
            assert seen[(g, layout)] >= want, (g, layout, seen[(g, layout)])
            # what the ranges say about the planted values (csrc/edfit_hist.inc: the bins' ends are exclusive)
            assert seen[(g, layout, "n=Kn-1")] == fc.FIRST and seen[(g, layout, "n=Kn+K2")] == fc.LIST
            assert seen[(g, layout, "y=Ky-1")] == fc.FIRST and seen[(g, layout, "y=Ky,small n")] == fc.LIST and seen[(g, layout, "y=Ky,large n")] == fc.LIST
            assert seen[(g, layout, "y=0")] == fc.FIRST and seen[(g, layout, "r=0")] == fc.FIRST and seen[(g, layout, "n=0")] == fc.SKIP
            assert seen[(g, layout, "n=Kn+K2-1")] == fc.LIST            # n = y + r < Kr + K2 - 1 inside both second-level ranges: the top n bin is never used
            if g != 2:
                assert seen[(g, layout, "n=Kn")] == (fc.MIXED if layout else fc.SECOND)          # r < Kr: the first level in k_fit_hist_sm
                assert seen[(g, layout, "r=Kr-1")] == (fc.MIXED if layout else fc.SECOND)
                assert seen[(g, layout, "r=Kr")] == fc.SECOND and seen[(g, layout, "r=R0+K2-1")] == fc.SECOND
                assert seen[(g, layout, "r=R0+K2")] == fc.LIST
            else:                                                                                  # K2 < Ky: R0 + K2 < Kr
                assert seen[(g, layout, "r=Kr-1")] == fc.LIST and seen[(g, layout, "r=Kr")] == fc.LIST
                assert seen[(g, layout, "r=R0+K2-1")] == fc.FIRST and seen[(g, layout, "r=R0+K2")] == fc.FIRST


def test_route_on_the_corners():
    """the restatement itself, on hand-worked cells of geometry 8 (Ky 1024, Kr = Kn 4096, R0 3072, K2 5120)"""
    cells = ((0, 0, "skip", "skip"), (1023, 3072, "first", "first"), (1023, 3073, "second", "mixed"), (1024, 100, "list", "list"),
             (0, 4095, "first", "first"), (0, 4096, "second", "second"), (1, 4095, "second", "mixed"), (10, 8191, "second", "second"),
             (10, 8192, "list", "list"), (1023, 8191, "second", "second"), (500, 3000, "first", "first"), (1023, 3071, "first", "first"),
             (900, 8191, "second", "second"), (0, 9215, "list", "list"))
    for y, r, l0, l1 in cells:
        assert fc.ROUTES[int(fc.route([y], [r], 8, 0)[0])] == l0 and fc.ROUTES[int(fc.route([y], [r], 8, 1)[0])] == l1, (y, r)
    # geometry 2 (Ky 4096, Kr = Kn 16384, R0 12288, K2 3072): k_fit_hist_sm has no second level of its own
    for y, r, want in ((4095, 12289, "second"), (1001, 15383, "list"), (1000, 15383, "first"), (2000, 14384, "second"), (1, 16383, "list")):
        assert fc.ROUTES[int(fc.route([y], [r], 2, 0)[0])] == want == fc.ROUTES[int(fc.route([y], [r], 2, 1)[0])], (y, r)


def test_region_follows_the_walks():
    E = 2 * 65535 + 2
    assert list(fc.region([0, 127, 128, 65534, 65535, 65536, 65537, 65536 + 65535], E, 8, 0)) == [0, 127, 0, 65534 % 128, 0, 128, 129, 128]
    assert list(fc.region([0, 3, 4, 1023, 1024, 2048, 2049, 2304], 2048 + 300, 8, 1, 4)) == [0, 0, 1, 255, 0, 0, 1, 0]
    assert list(fc.region([0, 7, 8, 2047, 2048, 2049], 2048 + 8, 8, 1, 8)) == [0, 0, 1, 255, 0, 1]
    assert list(fc.region([0, 1, 255, 256, 48127, 48128, 48129], 50000, 8, 1, 0)) == [0, 1, 255, 0, 48127 % 256, 0, 1]


def test_group_B_sits_on_the_capacity():
    kinds = {}
    for case in fc.group_B():
        g, layout = case.g, case.layout
        assert case.E == fc.E_B(g, layout) and fc.cap(case.E, g) == 8
        kind = case.name.split()[-1]
        col = case.cols[case.slot]
        counts = fc.list_counts(col.y, col.r, g, layout, case.vec)
        c = fc.cap(case.E, g)
        routes = fc.route(col.y, col.r, g, layout)
        if kind == "cap":
            assert counts.max() == c and (counts == c).sum() == 1 and not case.ran_out(case.slot)
        elif kind in ("cap+1", "pair"):
            assert counts.max() == c + 1 and (counts > c).sum() == 1 and case.ran_out(case.slot)
        elif kind == "all":
            assert (routes == fc.LIST).all() and (counts[:(fc.GEO[g].G if layout == 0 else fc.HS_BLOCK)] > c).all()
        elif kind == "second":
            assert not case.ran_out(case.slot) and (routes == fc.LIST).sum() == 0 and (routes == fc.SECOND).sum() >= case.E // 8
            assert (counts.sum() > 0) == (layout == 0 or g == 2)          # lists filled by the histogram kernel, emptied by the Newton kernel
        else:
            assert kind == "interleaved" and not case.ran_out(case.slot)
            target = fc.GEO[g].rows - 1 if layout == 0 else 77
            rows = np.flatnonzero(fc.region(np.arange(case.E), case.E, g, layout, case.vec) == target)[:c]
            assert list(routes[rows]) == [fc.SECOND, fc.LIST] * (c // 2)
        if kind == "pair":
            assert [case.ran_out(s) for s in range(case.S)] == [False, True, False, False] and case.S == fc.HN_S
        else:
            assert not case.ran_out(0) and not case.ran_out(2)
        kinds.setdefault((g, layout), set()).add(kind)
    assert all(kinds[(g, layout)] == set(fc.B_KINDS) | {"pair"} for g in fc.GEOMETRIES for layout in (0, 1))


def test_group_C_has_every_length_and_both_walks():
    cases = fc.group_C()
    for g, Es in fc.C_ROWS_0:
        assert {c.E for c in cases if c.g == g and c.layout == 0 and c.by == 1} >= set(Es)
    chunked = [c for c in cases if "(chunks)" in c.name]
    assert [c.E for c in chunked] == [131069, 131070, 131071, 131072, 262143] and all(c.S == 3 for c in chunked)
    for c in chunked:
        col = c.cols[1]
        assert np.all(col.r == col.r[0]) and len(np.unique(col.y)) > 100        # r constant: its bin holds 65 535 at the flush of every full chunk
        assert not c.ran_out(1)
    walks = {}
    for c in cases:
        if c.layout == 1:
            v = fc.in_vector_walk(np.arange(c.rows), c.rows, c.vec)
            walks.setdefault((c.bits, c.by), set()).add(("vector" if v.any() else "") + ("+scalar" if not v.all() else ""))
            if c.bits == 16 and c.by == 1 and c.E > 8 and "pitch" not in c.name:
                assert int((c.cols[1].y.astype(np.int64) + c.cols[1].r).max()) == 65535, c.name
    for bits in (32, 16):
        assert {c.E for c in cases if c.layout == 1 and c.bits == bits and c.by == 1} >= set(fc.C_ROWS_1 + fc.C_ROWS_1V + fc.C_CHUNK_1)
        assert walks[(bits, 1)] == {"vector", "vector+scalar", "+scalar"}, walks
    for bits, E in fc.C_PITCH:
        c = [c for c in cases if c.E == E and c.bits == bits and "pitch" in c.name][0]
        assert c.vec == 0 and E % (4 if bits == 32 else 8) != 0 and E > (fc.SPAN32 if bits == 32 else fc.SPAN16)
    assert {(c.by, c.layout) for c in cases if c.by > 1} == {(2, 0), (2, 1), (7, 0), (7, 1)}
    assert all(c.E % c.by != 0 and c.rows == (c.E - 1) // c.by + 1 for c in cases if c.by > 1)


def test_group_D_counts_its_early_movers():
    got = {}
    for case in fc.group_D():
        col = case.cols[0]
        assert (case.g, case.layout, case.S) == (8, 1, 2)
        got[case.name] = fc.carries(col.y, col.r, 8)
        assert not case.ran_out(1)                              # (a long ordinary column moves a few bins too: that is the kernel's everyday)
        assert case.ran_out(0) == (got[case.name][0] > fc.SM_CARRY)
    assert got["D 16383|16384"] == (3, fc.SM_HOT)             # one plateau's y, r and n bins at 16 384: they leave; the other's at 16 383: they stay
    col = fc.hot_column("16383|16384")
    first = col.y[:fc.SM_CHUNK].astype(np.int64) * 100000 + col.r[:fc.SM_CHUNK]
    assert sorted(np.unique(first, return_counts=True)[1])[-2:] == [fc.SM_HOT - 1, fc.SM_HOT]
    assert got["D 64511"] == (3, fc.SM_HOT - 1 + fc.SM_CHUNK) and got["D 64511"][1] == 64511
    assert got["D ('carries', 128)"][0] == 128 and got["D ('carries', 129)"][0] == 129
    assert all(top <= 65535 for _, top in got.values())
    # a single chunk is never looked at: no early mover in groups A and B
    assert all(fc.carries(c.y, c.r, case.geometry)[0] == 0 for case in fc.group_A() + fc.group_B() if case.layout == 1 for c in case.cols)


def test_groups_E_F_G_are_what_they_say():
    for g, widths in fc.E_WIDTHS:
        cases = [c for c in fc.group_E() if c.g == g]
        assert tuple(c.S for c in cases) == widths and all(c.E == 1024 for c in cases)
        for c in cases:
            assert len({col.key for col in c.cols}) == c.S                   # every column is different
    assert {fc.per_xcd(c.S, 8) for c in fc.group_E() if c.g == 8} == {1, 2, 3}
    for case in fc.group_F():
        depths = [fc.depth_of(c.y, c.r, case.layout) for c in case.cols]
        d = int(case.name.split()[-1])
        assert max(depths) == depths[case.slot] == d and sorted(depths)[-2] < fc.DEPTH_8 and case.runs == fc.geometry_of(d)
    assert [fc.geometry_of(d) for d in fc.F_DEPTHS] == [8, 4, 4, 2]
    for layout in (0, 1):
        seq = fc.F_sequence(layout)
        assert [fc.geometry_of(max(fc.depth_of(c.y, c.r, layout) for c in case.cols)) for case in seq] == [8, 2, 8]
    for case in fc.group_G():
        zeros, one = case.cols[1], case.cols[3]
        assert not zeros.y.any() and not zeros.r.any() and int(((one.y + one.r) > 0).sum()) == 1
        assert 8 in fc.moment_rows(case.E, case.layout) and one.y[8] > 0


# ---- conditions, by the checker alone -----------------------------------------------------------------------------------------------------

_MLE = {}


def _mle(oracle, y, r):
    key = (len(y), hash(y.tobytes()), hash(r.tobytes()))
    if key not in _MLE:
        _MLE[key] = oracle.fit_mle_hist(y, r)
    return _MLE[key]


def _bars(col, phi):
    if col.bar == "hot":
        return HOT_BARS
    t = FIT_REL_TOL * max(1.0, 2e-6 / (phi * phi))        # _check_mle's scaling
    return t, t


def _shift(oracle, col, y, r):
    """how far the checker's MLE of (y, r) is from that of the column, in units of the column's bar"""
    phi0, p0 = _mle(oracle, col.y, col.r)[:2]
    phi, p = oracle.fit_mle_hist(y, r)[:2]
    bphi, bp = _bars(col, phi0)
    return max(abs(phi - phi0) / phi0 / bphi, abs(p - p0) / p0 / bp)


def _held(cases):
    seen = set()
    for case in cases:
        for col in case.cols:
            if col.held and (col.key, case.layout) not in seen:
                seen.add((col.key, case.layout))
                yield case, col


SMALLEST = {}


@pytest.mark.parametrize("group", ["A", "B", "C", "D", "E", "F", "G"])
def test_every_held_column_is_well_conditioned_and_sensitive(oracle, group):
    """(i) the checker converges with phi >= 3e-3 and its two forms agree to 1e-9 (columns of up to 10 000 rows); (ii) its MLE moves by more
    than 1000 bars when the planted cells move by one count, when one cell is lost (group D: the cells of one early mover -- a single cell of
    10^6 cannot show at that group's 1e-6) and when the first half or chunk is counted twice"""
    cases = getattr(fc, "group_" + group)() + (fc.F_sequence(0) + fc.F_sequence(1) if group == "F" else ())
    n = 0
    for case, col in _held(cases):
        phi, p, ll, it = _mle(oracle, col.y, col.r)
        assert np.isfinite(phi) and np.isfinite(p) and np.isfinite(ll) and 0 < it < 50 and phi >= PHI_MIN and 0 < p < 1, (case.name, col.name, phi, p, it)
        if len(col.y) <= 10000:
            phi1, p1 = oracle.fit_mle(col.y, col.r)[:2]
            assert abs(phi1 - phi) <= 1e-9 * phi and abs(p1 - p) <= 1e-9 * p, (case.name, col.name)
        got = {"moved": _shift(oracle, col, *col.moved()), "dropped": _shift(oracle, col, *col.dropped()),
               "twice": _shift(oracle, col, *col.twice(case.layout))}
        for what, v in got.items():
            assert v > SENSITIVE, (case.name, col.name, what, v)
            SMALLEST[what] = min(SMALLEST.get(what, np.inf), v)
            SMALLEST[(group, what)] = min(SMALLEST.get((group, what), np.inf), v)
        n += 1
    assert n > 0
    print("group %s: %d columns; smallest shift in bars: %s" % (group, n, {w: "%.3g" % SMALLEST[(group, w)] for w in ("moved", "dropped", "twice")}))


@pytest.mark.parametrize("group", ["A", "B"])
def test_fit_mode_1_columns_show_a_lost_class(oracle, group):
    """the columns fit mode 1 is run on (planted share one half): the checker's own Nelder-Mead result (oracle.fit_nm) ends cleanly and moves by
    more than 10 x the bars of tests/test_gpu_fit_concordance.py when the planted class is removed"""
    cases = fc.group_A(0.5) if group == "A" else fc.group_B(0.5)
    seen, smallest = set(), np.inf
    for case in cases:
        col = case.cols[case.slot]
        if col.key in seen or col.name == "n=0":           # (cells without a read carry nothing: no class to lose)
            continue
        seen.add(col.key)
        phi, p, ne, fail = oracle.fit_nm(col.y, col.r, with_status=True)
        assert fail == 0 and 0 < phi < 1 and 0 < p < 1, (case.name, phi, p, fail)
        keep = np.setdiff1d(np.arange(len(col.y)), col.planted)
        phi1, p1, _, fail1 = oracle.fit_nm(col.y[keep], col.r[keep], with_status=True)
        v = max(abs(phi1 - phi) / phi / NM_BARS[0], abs(p1 - p) / p / NM_BARS[1])
        assert fail1 == 0 and v > 10.0, (case.name, v)
        smallest = min(smallest, v)
    print("group %s, fit mode 1: %d columns; smallest shift with the planted class removed: %.3g bars" % (group, len(seen), smallest))
