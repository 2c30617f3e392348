"""The host side of the annotation join (no GPU): the checker's two forms agree, the reference's quirks (R/annotate_extra.R:63-65) are pinned
by hand-written cases, the C-ABI's new symbols are bound, the name joining of AnnotateExtra, and no silent CPU path."""
import os
import re

import numpy as np
import pytest

import annot_checker as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ((False, False), (True, False), (False, True), (True, True))


def _run(form, S, Q, mo, fg=False, fk=False):
    return form(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"], mo,
                s_group=S.get("group") if fg else None, q_group=Q.get("group") if fg else None,
                s_kind=S.get("kind") if fk else None, q_kind=Q.get("kind") if fk else None)


def test_the_two_checker_forms_agree():
    n_hits = 0
    for name, S, Q in ac.cases(3):
        for mo in (0.0, 0.5, 1.0):
            for fg, fk in (FILTERS if "group" in S and "group" in Q else FILTERS[:1]):
                a, b = _run(ac.brute, S, Q, mo, fg, fk), _run(ac.windowed, S, Q, mo, fg, fk)
                for x, y in zip(a, b):
                    assert np.array_equal(x, y), (name, mo, fg, fk)
                n_hits += int(a[0].sum())
    assert n_hits > 1000          # the generator's cases are not trivially empty


def test_window_widths_of_the_built_shapes():
    for w in (1, 31, 32, 33, 200):
        S = ac.stack(w)
        assert ac.window_widths(S["chrom"], S["start"], S["end"], [0], [1000], [2000]).tolist() == [w]
        assert _run(ac.brute, S, {"chrom": [0], "start": [1000], "end": [2000]}, 0.5)[0].tolist() == [w]
        S = ac.stack(w, n_survive=w // 2)
        assert _run(ac.brute, S, {"chrom": [0], "start": [1000], "end": [2000]}, 0.5)[0].tolist() == [w // 2]
        S = ac.shadowed(w + 1)
        Q = {"chrom": [0], "start": [100000], "end": [101000]}
        assert ac.window_widths(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"]).tolist() == [w + 1]
        assert _run(ac.brute, S, Q, 0.0)[0].tolist() == [0]


def _one(qs, qe, ss, se, mo):
    """hits of the single query [qs, qe] against the single subject [ss, se], both forms"""
    S = {"chrom": [0], "start": [ss], "end": [se]}
    Q = {"chrom": [0], "start": [qs], "end": [qe]}
    a, b = _run(ac.brute, S, Q, mo), _run(ac.windowed, S, Q, mo)
    assert a[0].tolist() == b[0].tolist()
    return int(a[0][0])


def test_quirks_of_the_overlap_formula():
    # qs == qe: ov <= 0 and the bar is 0: never annotated, whatever covers it
    assert _one(500, 500, 0, 1000, 0.0) == 0 and _one(500, 500, 500, 500, 0.0) == 0
    # a subject touching the call in one base: ov = 0
    assert _one(100, 200, 200, 300, 0.0) == 0 and _one(100, 200, 50, 100, 0.0) == 0
    # min_overlap = 0: two bases or more count (ov = 1 > 0)
    assert _one(100, 200, 199, 300, 0.0) == 1 and _one(100, 200, 50, 101, 0.0) == 1
    # a subject equal to the call, or covering it: ov == qe - qs, a hit below 1 and not at 1
    assert _one(100, 200, 100, 200, 0.5) == 1 and _one(100, 200, 100, 200, 0.999) == 1 and _one(100, 200, 100, 200, 1.0) == 0
    assert _one(100, 200, 0, 1000, 1.0) == 0
    # min_overlap = 1 admits nothing at all (ov <= qe - qs); above 1 neither
    assert _one(100, 200, 101, 199, 1.0) == 0
    # exactly half is not "more than half": ov = 50 of a length-100 call
    assert _one(100, 200, 150, 400, 0.5) == 0 and _one(100, 200, 149, 400, 0.5) == 1
    # disjoint ranges never reach the overlap test
    assert _one(100, 200, 201, 300, 0.0) == 0 and _one(100, 200, 0, 99, 0.0) == 0


def test_comparison_is_one_binary64_product_and_compare():
    """0.7 * 90.0 is 62.99999999999999 in binary64 (the real product is 63): ov = 63 IS a hit.  0.55 * 100.0 is 55.00000000000001: ov = 55 is
    not, ov = 56 is.  Both sides differ in the last bit only; an implementation that scales, fuses or reorders would flip the first."""
    assert np.float64(0.7) * np.float64(90) == np.nextafter(np.float64(63), -np.inf)
    assert np.float64(0.55) * np.float64(100) == np.nextafter(np.float64(55), np.inf)
    assert _one(1000, 1090, 1000, 1063, 0.7) == 1          # ov = 63
    assert _one(1000, 1090, 1000, 1062, 0.7) == 0          # ov = 62
    assert _one(1000, 1100, 1000, 1055, 0.55) == 0         # ov = 55
    assert _one(1000, 1100, 1000, 1056, 0.55) == 1         # ov = 56


def test_order_within_a_query_and_filters():
    S = {"chrom": [0, 0, 0, 0, 1], "start": [50, 10, 50, 10, 10], "end": [500, 500, 500, 500, 500],
         "group": [0, 1, 2, 1, 0], "kind": [1, 1, 2, 2, 1]}
    Q = {"chrom": [0], "start": [100], "end": [200], "group": [1], "kind": [1]}
    for form in (ac.brute, ac.windowed):
        assert _run(form, S, Q, 0.5)[2].tolist() == [1, 3, 0, 2]                 # (start, index); the other chromosome never
        assert _run(form, S, Q, 0.5, fg=True)[2].tolist() == [0, 2]             # own group dropped
        assert _run(form, S, Q, 0.5, fk=True)[2].tolist() == [1, 0]             # same kind kept
        assert _run(form, S, Q, 0.5, fg=True, fk=True)[2].tolist() == [0]


def test_name_joining_of_annotate_extra():
    from exomedepth_amd import api
    names = np.array(["geneA", "geneB", 7, "geneD"], dtype=object)
    offsets = np.array([0, 2, 2, 3, 6], np.int64)
    hits = np.array([3, 0, 1, 2, 2, 0], np.int32)
    want = ["geneD,geneA", None, "geneB", "7,7,geneA"]                           # "," , None for no hit, the hit list's order kept
    assert api._join_hit_names(names, offsets, hits) == want
    assert ac.names_column(names, offsets, hits) == want
    assert api._join_hit_names(names, np.zeros(1, np.int64), np.zeros(0, np.int32)) == []


def test_new_symbols_are_declared_and_bound():
    from exomedepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("ed_annot_create", "ed_annot_destroy", "ed_annot_n", "ed_annot_overlaps", "ed_annot_geometry"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound, name
    import exomedepth_amd as ed
    for name in ("Annotation", "annotate_calls", "cohort_call_recurrence"):
        assert hasattr(ed, name) and name in ed.__all__
    assert hasattr(ed.ExomeDepth, "AnnotateExtra")


def test_no_device_no_annotation():
    import __graft_entry__ as g
    g.build()
    import exomedepth_amd as ed
    from exomedepth_amd import _lib
    if _lib.lib().ed_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(ed.EdError, match="no usable HIP device"):
        ed.Annotation(["1", "1"], [10, 20], [15, 30])
    with pytest.raises(ed.EdError, match="no usable HIP device"):
        calls = np.zeros(2, dtype=ed.api.CALL_DTYPE)
        ed.cohort_call_recurrence(calls, ["1"], [10, 20], [15, 30])


def test_bad_intervals_are_refused_before_any_device_work():
    """the argument checks come first: they answer ED_ERR_INVALID with or without a device"""
    import __graft_entry__ as g
    g.build()
    import exomedepth_amd as ed
    for start, end in (([-1], [5]), ([9], [8])):
        with pytest.raises(ed.EdError, match="0 <= start <= end"):
            ed.Annotation(["1"], start, end)
    with pytest.raises(ValueError):
        ed.Annotation(["1"], [0], [2**31])
    with pytest.raises(ValueError):
        ed.Annotation(["1"], [0.5], [3])
