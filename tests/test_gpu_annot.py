"""The annotation join on the device (csrc/edannot.inc: ed_annot_*, api.Annotation / AnnotateExtra / annotate_calls / cohort_call_recurrence)
against tests/annot_checker.py's brute-force statement of R/annotate_extra.R:43-71.  Every comparison is exact equality of counts, offsets,
the total and the WHOLE hits array: the rule is one binary64 product and one compare of exactly represented integers, so there is no tolerance
and no cell is left out.  Shapes sit on the kernels' edges (ed_annot_geometry): the lane / wave threshold, the workgroup sizes, the scan block."""
import ctypes as C
import os

import numpy as np
import pytest

import annot_checker as ac

pytestmark = pytest.mark.gpu

FILTERS = ((False, False), (True, False), (False, True), (True, True))
SENTINEL = -77


def _names(ids):
    return ["c%d" % int(i) for i in np.asarray(ids).ravel()]


def _track(ed, S, groups=True):
    return ed.Annotation(_names(S["chrom"]), S["start"], S["end"], group=S.get("group") if groups else None,
                         kind=S.get("kind") if groups else None)


def _want(S, Q, mo, fg=False, fk=False):
    return ac.brute(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"], mo,
                    s_group=S["group"] if fg else None, q_group=Q["group"] if fg else None,
                    s_kind=S["kind"] if fk else None, q_kind=Q["kind"] if fk else None)


def _got(track, Q, mo, fg=False, fk=False, n=None):
    sl = slice(0, n)
    return track.overlaps(_names(np.asarray(Q["chrom"])[sl]), np.asarray(Q["start"])[sl], np.asarray(Q["end"])[sl], min_overlap=mo,
                          group=np.asarray(Q["group"])[sl] if fg else None, kind=np.asarray(Q["kind"])[sl] if fk else None)


def _same(got, want, what=""):
    for g, w, nm in zip(got, want, ("counts", "offsets", "hits")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, nm, g.shape, w.shape)
        assert np.array_equal(g, w), (what, nm, np.nonzero(g != w)[0][:5])


@pytest.fixture(scope="module")
def geo(edlib):
    return edlib.annot_geometry()


@pytest.fixture(scope="module")
def big(geo):
    """one shuffled track -- 64, 65, 0, 1000, 1, 2 subjects on chromosomes 0 .. 5 (an empty one in the middle) -- and 2 * scan block + 1 queries on
    chromosomes -1 .. 6 (two of them on the query side only), with the checker's answers under the four filter settings: made once, never changed"""
    rng = np.random.default_rng(11)
    S = ac.random_set(rng, [64, 65, 0, 1000, 1, 2])
    Q = ac.random_queries(rng, 2 * geo["scan_block"] + 1, 6)
    want = {(fg, fk): _want(S, Q, 0.5, fg, fk) for fg, fk in FILTERS}
    widths = ac.window_widths(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"])
    assert widths.min() == 0 and widths.max() > 4 * geo["wave_pass"] and np.sum(widths <= geo["wide_threshold"]) > 100     # both kernel forms in one launch
    return S, Q, want


@pytest.mark.parametrize("fg,fk", FILTERS, ids=["nofilter", "group", "kind", "group+kind"])
def test_whole_set_and_filters(edlib, big, fg, fk):
    S, Q, want = big
    t = _track(edlib, S)
    try:
        _same(_got(t, Q, 0.5, fg, fk), want[(fg, fk)])
    finally:
        t.close()
    assert want[(fg, fk)][0].sum() > 1000


def test_query_counts_at_the_workgroup_and_scan_edges(edlib, big, geo):
    """0, 1, 63, 64, 65, one below / at / above the lane form's workgroup and the scan's block, and two scan blocks + 1: a prefix of the query set
    must give the prefix of the answer"""
    S, Q, want = big
    counts, offsets, hits = want[(False, False)]
    B, SB = geo["queries_per_workgroup"], geo["scan_block"]
    t = _track(edlib, S)
    try:
        for n in sorted({0, 1, 63, 64, 65, B - 1, B, B + 1, SB - 1, SB, SB + 1, 2 * SB, 2 * SB + 1}):
            _same(_got(t, Q, 0.5, n=n), (counts[:n], offsets[:n + 1], hits[:offsets[n]]), "n_q = %d" % n)
    finally:
        t.close()


def test_window_widths_at_the_lane_wave_threshold(edlib, geo):
    """windows one below, at and one above the threshold, at and around the wave's 64-subject pass, wider than a workgroup's four passes, and 1 000:
    every candidate surviving, a third surviving, and the wide window with NO survivor (a long early subject lifts the running maximum)"""
    W, P = geo["wide_threshold"], geo["wave_pass"]
    widths = sorted({1, 2, W - 1, W, W + 1, P - 1, P, P + 1, 4 * P - 1, 4 * P, 4 * P + 1, 1000})
    parts, qs = [], []
    for k, w in enumerate(widths):
        for j, S in enumerate((ac.stack(w, chrom=3 * k), ac.stack(w, n_survive=w // 3, chrom=3 * k + 1), ac.shadowed(w, chrom=3 * k + 2))):
            parts.append(S)
            q = (1000, 2000) if j < 2 else (100000, 101000)
            qs.append((3 * k + j, q[0], q[1]))
    S = {k: np.concatenate([p[k] for p in parts]) for k in ("chrom", "start", "end")}
    rng = np.random.default_rng(5)
    perm = rng.permutation(S["chrom"].size)
    S = {k: v[perm] for k, v in S.items()}
    Q = {"chrom": np.array([q[0] for q in qs]), "start": np.array([q[1] for q in qs]), "end": np.array([q[2] for q in qs])}
    got_w = ac.window_widths(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"])
    assert got_w.tolist() == [w for w in widths for _ in range(3)]                 # the shapes are what they claim to be
    want = _want(S, Q, 0.5)
    assert want[0].tolist() == [x for w in widths for x in (w, w // 3, 0)]
    t = _track(edlib, S)
    try:
        _same(_got(t, Q, 0.5), want)
        # the same queries 5 times over, interleaved with narrow ones: lane and wave form in the same launch, more wide queries than one workgroup has waves
        rep = {k: np.concatenate([np.tile(v, 5), v[:7]]) for k, v in Q.items()}
        _same(_got(t, rep, 0.5), _want(S, rep, 0.5))
        _same(_got(t, Q, 0.0), _want(S, Q, 0.0))
    finally:
        t.close()


def test_identical_starts_break_ties_by_index(edlib, geo):
    rng = np.random.default_rng(2)
    n = 3 * geo["wave_pass"] + 5
    S = {"chrom": np.zeros(n, np.int64), "start": np.full(n, 5000), "end": 5000 + rng.integers(0, 3000, n)}
    S["start"][rng.random(n) < 0.2] = 4000
    Q = {"chrom": [0, 0, 0], "start": [5000, 4500, 3000], "end": [6000, 5200, 9000]}
    want = _want(S, Q, 0.3)
    assert want[0].max() > 2 * geo["wave_pass"] and want[0].min() > 0
    for q in range(3):
        h = want[2][want[1][q]:want[1][q + 1]]
        st = S["start"][h]
        assert np.all((st[1:] > st[:-1]) | ((st[1:] == st[:-1]) & (h[1:] > h[:-1])))
    t = _track(edlib, S, groups=False)
    try:
        _same(_got(t, Q, 0.3), want)
    finally:
        t.close()


def test_edges_of_the_coordinate_range_and_of_a_chromosome(edlib):
    I = ac.IMAX
    S = {"chrom": [0, 0, 0, 0, 2, 2], "start": [0, 0, I - 5, I, 100, 300], "end": [0, I, I, I, 200, 300]}       # chromosome 1 empty; start == end subjects
    Q = {"chrom": [0, 0, 0, 0, 2, 2, 2, 1, 3, -1], "start": [0, 0, I - 9, I, 0, 301, 150, 5, 5, 5], "end": [I, 7, I, I, 99, 400, 300, 50, 50, 50]}
    t = _track(edlib, S, groups=False)
    try:
        for mo in (0.0, 0.5, 1.0):
            _same(_got(t, Q, mo), _want(S, Q, mo), mo)
    finally:
        t.close()
    assert _want(S, Q, 0.0)[0].tolist() == [2, 1, 2, 0, 0, 0, 1, 0, 0, 0]


def test_quirks_on_the_device(edlib):
    """the hand-written cases of tests/test_annot_host.py, last-bit products included, through the kernels"""
    S = {"chrom": [0] * 8, "start": [0, 500, 200, 199, 1000, 1000, 1000, 1000], "end": [1000, 500, 300, 300, 1063, 1062, 1055, 1056]}
    t = _track(edlib, S, groups=False)
    try:
        for Q, mo in (({"chrom": [0, 0], "start": [500, 100], "end": [500, 200]}, 0.0),
                      ({"chrom": [0, 0], "start": [100, 0], "end": [200, 1000]}, 1.0),
                      ({"chrom": [0, 0], "start": [0, 100], "end": [1000, 200]}, 0.999),
                      ({"chrom": [0], "start": [1000], "end": [1090]}, 0.7),
                      ({"chrom": [0], "start": [1000], "end": [1100]}, 0.55)):
            _same(_got(t, Q, mo), _want(S, Q, mo), mo)
    finally:
        t.close()
    assert _want(S, {"chrom": [0], "start": [1000], "end": [1090]}, 0.7)[2].tolist() == [4]                 # ov = 63 > 62.99999999999999; 62, 56, 55 are not
    assert _want(S, {"chrom": [0], "start": [1000], "end": [1100]}, 0.55)[2].tolist() == [4, 5, 7]          # ov = 55 is not > 55.00000000000001; 56, 62, 63 are


def test_no_subjects_and_no_queries(edlib):
    empty = {"chrom": np.zeros(0, np.int64), "start": np.zeros(0, np.int64), "end": np.zeros(0, np.int64)}
    Q = {"chrom": [0, 1], "start": [5, 5], "end": [50, 50]}
    t = _track(edlib, empty, groups=False)
    try:
        assert t.n == 0
        _same(_got(t, Q, 0.5), _want(empty, Q, 0.5))
        _same(_got(t, empty, 0.5), _want(empty, empty, 0.5))
    finally:
        t.close()


def test_empty_chromosomes_in_the_middle_at_the_c_level(edlib):
    """ids 1, 2 and 4 of 5 have no subject (Annotation only makes ids for names it has seen, so this goes through the C entry)"""
    L = edlib._lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    S = {"chrom": np.array([3, 0, 3, 0, 3]), "start": np.array([50, 10, 5, 10, 60]), "end": np.array([90, 40, 70, 12, 60])}
    Q = {"chrom": [0, 1, 2, 3, 4, 5, 3], "start": [0, 0, 0, 0, 0, 0, 55], "end": [100, 100, 100, 100, 100, 100, 65]}
    h = C.c_void_p()
    arrs = [np.ascontiguousarray(S[k], dtype=np.int32) for k in ("chrom", "start", "end")]
    assert L.ed_annot_create(C.byref(h), 0, 5, 5, *(p(a) for a in arrs), None, None) == 0
    try:
        assert L.ed_annot_n(h) == 5
        want = _want(S, Q, 0.2)
        buf = np.full(int(want[1][-1]), SENTINEL, np.int32)
        rc, c, o, n, msg = _raw(edlib, h, Q, 0.2, hits=buf, cap=buf.size)
        assert rc == 0, msg
        _same((c, o, buf), want)
        assert want[0].tolist() == [1, 0, 0, 2, 0, 0, 2]
    finally:
        L.ed_annot_destroy(h)


def test_self_join_never_hits_the_own_sample(edlib):
    rng = np.random.default_rng(8)
    n = 700
    S = ac.random_set(rng, [n, 40], span=4000, n_groups=12)
    t = _track(edlib, S)
    try:
        for fk in (False, True):
            got = _got(t, S, 0.5, True, fk)
            _same(got, _want(S, S, 0.5, True, fk), fk)
            q_of = np.repeat(np.arange(S["chrom"].size), got[0])
            assert np.all(S["group"][got[2]] != S["group"][q_of]) and np.all(got[2] != q_of)
            assert got[0].max() > 64
    finally:
        t.close()


# ---- the C protocol --------------------------------------------------------------------------------------------------------------------
def _raw(ed, handle, Q, mo, hits=None, cap=0, group=None, kind=None, want_offsets=True):
    L = ed._lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    qc, qs, qe = (np.ascontiguousarray(Q[k], dtype=np.int32) for k in ("chrom", "start", "end"))
    n = qs.size
    counts, offsets, total = np.full(n, -1, np.int64), np.full(n + 1, -1, np.int64), C.c_int64(-1)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    k = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    rc = L.ed_annot_overlaps(handle, n, p(qc), p(qs), p(qe), None if g is None else p(g), None if k is None else p(k), float(mo), p(counts),
                             p(offsets) if want_offsets else None, None if hits is None else p(hits), cap, C.byref(total))
    return rc, counts, offsets, total.value, L.ed_last_error().decode()


def test_count_only_cap_too_small_and_exact(edlib, big):
    S, Q, want = big
    counts, offsets, hits = want[(False, False)]
    total = int(offsets[-1])
    t = _track(edlib, S)
    try:
        Qi = {"chrom": t.chromosome_ids(_names(Q["chrom"])), "start": Q["start"], "end": Q["end"]}
        rc, c, o, n, _ = _raw(edlib, t.handle, Qi, 0.5)                                     # hits = NULL: count only
        assert rc == 0 and n == total and np.array_equal(c, counts) and np.array_equal(o, offsets)
        rc, c, o, n, _ = _raw(edlib, t.handle, Qi, 0.5, want_offsets=False)
        assert rc == 0 and n == total and np.array_equal(c, counts)
        buf = np.full(total + 8, SENTINEL, np.int32)
        rc, c, o, n, msg = _raw(edlib, t.handle, Qi, 0.5, hits=buf, cap=total - 1)          # one too small
        assert rc == -1 and n == total and str(total) in msg
        assert np.all(buf == SENTINEL) and np.array_equal(c, counts) and np.array_equal(o, offsets)
        rc, c, o, n, _ = _raw(edlib, t.handle, Qi, 0.5, hits=buf, cap=total)                # exact
        assert rc == 0 and n == total and np.array_equal(buf[:total], hits) and np.all(buf[total:] == SENTINEL)
    finally:
        t.close()


def test_one_track_many_query_sets_and_two_tracks_alive(edlib, big):
    S, Q, want = big
    rng = np.random.default_rng(21)
    S2 = ac.random_set(rng, [30, 200])
    a, b = _track(edlib, S), _track(edlib, S2)
    try:
        for i, mo in enumerate((0.0, 0.25, 0.5, 1.0, 0.5)):
            Qi = ac.random_queries(rng, 150 + 400 * i, 6)
            _same(_got(a, Qi, mo, i % 2 == 1, i % 3 == 1), _want(S, Qi, mo, i % 2 == 1, i % 3 == 1), ("a", i))
            _same(_got(b, Qi, mo), _want(S2, Qi, mo), ("b", i))
        _same(_got(a, Q, 0.5), want[(False, False)])
    finally:
        a.close(); b.close()


def test_invalid_arguments(edlib):
    L = edlib._lib.lib()
    i32 = lambda *v: np.array(v, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    h = C.c_void_p()
    for chrom, start, end, n_chrom in ((i32(0), i32(-1), i32(5), 1), (i32(0), i32(9), i32(8), 1), (i32(1), i32(1), i32(2), 1), (i32(-1), i32(1), i32(2), 1)):
        assert L.ed_annot_create(C.byref(h), 0, 1, n_chrom, p(chrom), p(start), p(end), None, None) == -1 and not h.value
    assert L.ed_annot_create(None, 0, 0, 0, None, None, None, None, None) == -1
    assert L.ed_annot_create(C.byref(h), 0, -1, 1, None, None, None, None, None) == -1
    assert L.ed_annot_create(C.byref(h), 0, 1, 1, None, None, None, None, None) == -1
    S = {"chrom": [0, 0], "start": [10, 20], "end": [30, 40]}
    plain, full = _track(edlib, S, groups=False), _track(edlib, dict(S, group=[0, 1], kind=[1, 2]))
    try:
        ok = {"chrom": [0], "start": [5], "end": [50]}
        assert _raw(edlib, full.handle, ok, 0.5, group=[0], kind=[1])[0] == 0
        for bad in (float("nan"), float("inf"), -0.5, -float("inf")):
            assert _raw(edlib, plain.handle, ok, bad)[0] == -1
        assert _raw(edlib, plain.handle, {"chrom": [0], "start": [-1], "end": [50]}, 0.5)[0] == -1
        assert _raw(edlib, plain.handle, {"chrom": [0], "start": [51], "end": [50]}, 0.5)[0] == -1
        assert _raw(edlib, plain.handle, ok, 0.5, group=[0])[0] == -1                       # a filter the track has no array for
        assert _raw(edlib, plain.handle, ok, 0.5, kind=[1])[0] == -1
        buf = np.full(4, SENTINEL, np.int32)
        assert _raw(edlib, plain.handle, ok, 0.5, hits=buf, cap=-1)[0] == -1 and np.all(buf == SENTINEL)
        assert _raw(edlib, None, ok, 0.5)[0] == -1
        tot = C.c_int64()
        assert L.ed_annot_overlaps(plain.handle, 1, None, None, None, None, None, 0.5, None, None, None, 0, C.byref(tot)) == -1
        assert L.ed_annot_overlaps(plain.handle, -1, None, None, None, None, None, 0.5, None, None, None, 0, C.byref(tot)) == -1
        assert L.ed_annot_overlaps(plain.handle, 0, None, None, None, None, None, 0.5, None, None, None, 0, None) == -1
        assert _raw(edlib, plain.handle, ok, 0.25)[3] == 2                                  # and the object still works
        assert L.ed_annot_n(plain.handle) == 2 and L.ed_annot_n(None) == 0
    finally:
        plain.close(); full.close()
    with pytest.raises(edlib.EdError):
        plain.overlaps(["c0"], [5], [50])                                                   # closed


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_annotate_extra_on_the_bundled_data(edlib):
    """the reference's bundled counts through ExomeDepth(...).CallCNVs(...).AnnotateExtra(...): the annotation is the design's own exons named
    by index; the new column equals the checker's string for every call"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exomecount_chr1.npz"))
    start, end, counts = d["start"], d["end"], d["counts"]
    n = start.size
    x = edlib.ExomeDepth(counts[:, 0].astype(float), counts[:, 1:].sum(axis=1).astype(float))
    x.CallCNVs(["1"] * n, start, end, ["exon%d" % i for i in range(n)])
    assert len(x.CNV_calls) >= 20
    # the design holds a few zero-width rows (end == start - 1, an empty IRanges range); an annotation takes 0 <= start <= end only, so the track
    # is the design's other exons, still named by their index in the design
    ok = np.nonzero(end >= start)[0]
    assert n - 50 < ok.size < n
    start, end, n = start[ok], end[ok], ok.size
    names = np.array(["exon%d" % i for i in ok], dtype=object)
    track = edlib.Annotation(["1"] * n, start, end, names=names)
    other = edlib.Annotation(["chr1"] * n, start, end, names=names)                         # a different name: nothing matches
    try:
        for mo in (0.5, 0.01):
            assert x.AnnotateExtra(track, min_overlap=mo, column_name="exons.hg19") is x
            cs = np.array([c["start"] for c in x.CNV_calls]); ce = np.array([c["end"] for c in x.CNV_calls])
            z = np.zeros(cs.size, np.int64)
            _, off, hits = ac.brute(np.zeros(n, np.int64), start, end, z, cs, ce, mo)
            want = ac.names_column(names, off, hits)
            assert [c["exons.hg19"] for c in x.CNV_calls] == want
        assert any(w is not None and "," in w for w in want)                                # at 1 % a call of several exons lists them
        x.AnnotateExtra(other, column_name="none")
        assert all(c["none"] is None for c in x.CNV_calls)
    finally:
        track.close(); other.close()


def test_cohort_table_annotation_and_recurrence(edlib):
    """2 000 exons x 16 samples with a deletion planted in five samples over the same 31 exons: annotate_calls and cohort_call_recurrence on
    the cohort's own call table equal the checker, and the planted calls report the four other carriers"""
    from exomedepth_amd import synth
    E, S, C_ = 2000, 16, 4
    chrom_off, start, end = synth.exon_design(E, C_, 3)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, 3, n_segments=2, mean_depth=120.0)
    planted, lo, hi = (1, 4, 7, 10, 15), 700, 730
    test = test.copy()
    test[lo:hi + 1, planted] = test[lo:hi + 1, planted] // 2
    plan = edlib.Plan(chrom_off, start, end)
    co = edlib.Cohort(plan, 8, 2)
    try:
        out = co.run_host(test, ref, 0, phi=phi, expected=p)
    finally:
        co.close(); plan.close()
    calls = out["calls"]
    assert calls.size >= 15
    levels = ["%d" % (c + 1) for c in range(C_)]
    ecode = np.repeat(np.arange(C_), np.diff(chrom_off))
    names = np.array(["e%d" % i for i in range(E)], dtype=object)
    cc, cs, ce = calls["chrom"].astype(np.int64), start[calls["start_exon"]].astype(np.int64), end[calls["end_exon"]].astype(np.int64)
    track = edlib.Annotation([levels[c] for c in ecode], start, end, names=names)
    try:
        got = edlib.annotate_calls(calls, levels, start, end, track, min_overlap=0.1)
    finally:
        track.close()
    _same(got, ac.brute(ecode, start, end, cc, cs, ce, 0.1))
    sample, kind = calls["sample"].astype(np.int64), calls["type"].astype(np.int64)
    for same_type in (True, False):
        want = ac.brute(cc, cs, ce, cc, cs, ce, 0.5, s_group=sample, q_group=sample, s_kind=kind if same_type else None, q_kind=kind if same_type else None)
        n_calls, n_carriers = edlib.cohort_call_recurrence(calls, levels, start, end, min_overlap=0.5, same_type=same_type, carriers=True)
        assert n_calls.dtype == np.int64 and np.array_equal(n_calls, want[0])
        assert np.array_equal(n_carriers, ac.carriers(*want, sample))
        assert np.array_equal(edlib.cohort_call_recurrence(calls, levels, start, end, min_overlap=0.5, same_type=same_type), want[0])
    n_calls, n_carriers = edlib.cohort_call_recurrence(calls, levels, start, end, carriers=True)
    is_planted = np.isin(calls["sample"], planted) & (calls["type"] == 1) & (calls["start_exon"] <= lo + 3) & (calls["end_exon"] >= hi - 3) & \
        (calls["end_exon"] - calls["start_exon"] <= hi - lo + 6)
    assert sorted(calls["sample"][is_planted].tolist()) == list(planted)                    # each carrier has its call over the planted exons
    assert n_carriers[is_planted].tolist() == [len(planted) - 1] * len(planted)
