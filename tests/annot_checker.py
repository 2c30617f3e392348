"""Not a test: a numpy restatement of the reference's AnnotateExtra (R/annotate_extra.R:43-71) plus the library's two filters, the statement
the GPU join (csrc/edannot.inc) is compared with, cell for cell.

A query [qs, qe] on chromosome c and a subject [ss, se] on c' are a hit iff
    c == c'                                         seqnames match (:43-47)
    qs <= se and ss <= qe                           findOverlaps, type "any", closed integer ranges (:46)
    float(ov) > min_overlap * float(qe - qs)        ov = min(se, qe) - max(qs, ss): no + 1 (:63-65)
    group filter (when both groups are given): q_group != s_group;  kind filter (when both kinds are given): q_kind == s_kind
Hits of one query are ordered by (subject start, subject index): the library's definition (GenomicRanges orders by query only).

    brute(...)   O(n_q * n), one vectorised row per query: the statement of record
    windowed(...) subjects sorted by start per chromosome, candidates cut by searchsorted: for the larger inputs (tools/bench_annot.py times it)
    cases(seed)  a seeded generator of interval sets with the geometries the kernels can go wrong on
Chromosomes are integer ids here; a query id the subjects do not have simply matches nothing.
"""
import numpy as np


def _arr(x, dtype=np.int64):
    return np.asarray(x, dtype=dtype).ravel()


def _csr(per_query):
    counts = np.array([len(h) for h in per_query], dtype=np.int64)
    offsets = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    hits = np.concatenate(per_query).astype(np.int32) if counts.sum() else np.zeros(0, np.int32)
    return counts, offsets, hits


def _keep(qs, qe, ss, se, min_overlap):
    """the two tests of :46 and :63-65 on int64 arrays; one binary64 product, one compare"""
    ov = np.minimum(se, qe) - np.maximum(qs, ss)
    return (qs <= se) & (ss <= qe) & (ov.astype(np.float64) > np.float64(min_overlap) * np.float64(qe - qs))


def brute(s_chrom, s_start, s_end, q_chrom, q_start, q_end, min_overlap, s_group=None, q_group=None, s_kind=None, q_kind=None):
    """(counts, offsets, hits): every query against every subject"""
    sc, ss, se = _arr(s_chrom), _arr(s_start), _arr(s_end)
    qc, qs, qe = _arr(q_chrom), _arr(q_start), _arr(q_end)
    order = np.lexsort((np.arange(ss.size), ss))            # (start, index)
    fg = s_group is not None and q_group is not None
    fk = s_kind is not None and q_kind is not None
    sg, qg = (_arr(s_group), _arr(q_group)) if fg else (None, None)
    sk, qk = (_arr(s_kind), _arr(q_kind)) if fk else (None, None)
    out = []
    for q in range(qs.size):
        m = (sc == qc[q]) & _keep(qs[q], qe[q], ss, se, min_overlap)
        if fg:
            m &= sg != qg[q]
        if fk:
            m &= sk == qk[q]
        out.append(order[m[order]])
    return _csr(out)


def windowed(s_chrom, s_start, s_end, q_chrom, q_start, q_end, min_overlap, s_group=None, q_group=None, s_kind=None, q_kind=None):
    """the same by sorting: per chromosome the subjects in (start, index) order, a query's candidates those with start <= qe
    (searchsorted), cut below by the running maximum of the ends; then the same tests"""
    sc, ss, se = _arr(s_chrom), _arr(s_start), _arr(s_end)
    qc, qs, qe = _arr(q_chrom), _arr(q_start), _arr(q_end)
    fg = s_group is not None and q_group is not None
    fk = s_kind is not None and q_kind is not None
    sg, qg = (_arr(s_group), _arr(q_group)) if fg else (None, None)
    sk, qk = (_arr(s_kind), _arr(q_kind)) if fk else (None, None)
    out = [np.zeros(0, np.int64)] * qs.size
    for c in np.unique(qc):
        si = np.nonzero(sc == c)[0]
        if si.size == 0:
            continue
        si = si[np.argsort(ss[si], kind="stable")]
        st, en = ss[si], se[si]
        pmax = np.maximum.accumulate(en)
        for q in np.nonzero(qc == c)[0]:
            hi = np.searchsorted(st, qe[q], side="right")
            lo = np.searchsorted(pmax[:hi], qs[q], side="left")
            w = slice(lo, hi)
            m = _keep(qs[q], qe[q], st[w], en[w], min_overlap)
            if fg:
                m &= sg[si[w]] != qg[q]
            if fk:
                m &= sk[si[w]] == qk[q]
            out[q] = si[w][m]
    return _csr(out)


def window_widths(s_chrom, s_start, s_end, q_chrom, q_start, q_end):
    """number of candidates [lo, hi) the sort-and-window form looks at per query: what decides the kernel path on the device"""
    sc, ss, se = _arr(s_chrom), _arr(s_start), _arr(s_end)
    qc, qs, qe = _arr(q_chrom), _arr(q_start), _arr(q_end)
    out = np.zeros(qs.size, np.int64)
    for c in np.unique(qc):
        si = np.nonzero(sc == c)[0]
        if si.size == 0:
            continue
        si = si[np.argsort(ss[si], kind="stable")]
        pmax = np.maximum.accumulate(se[si])
        qi = np.nonzero(qc == c)[0]
        hi = np.searchsorted(ss[si], qe[qi], side="right")
        lo = np.minimum(np.searchsorted(pmax, qs[qi], side="left"), hi)
        out[qi] = hi - lo
    return out


def names_column(names, offsets, hits):
    """what AnnotateExtra writes (:67-71): the hits' names pasted with ",", None (NA) for a call without hits"""
    return [",".join(str(names[h]) for h in hits[offsets[q]:offsets[q + 1]]) if offsets[q + 1] > offsets[q] else None
            for q in range(len(offsets) - 1)]


def carriers(counts, offsets, hits, s_group):
    """distinct groups among each query's hits"""
    g = _arr(s_group)
    return np.array([np.unique(g[hits[offsets[q]:offsets[q + 1]]]).size for q in range(counts.size)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------
IMAX = 2**31 - 1


def random_set(rng, n_per_chrom, span=20000, max_len=400, n_groups=7):
    """subjects over chromosomes 0 .. len(n_per_chrom) - 1 (entries may be 0: empty chromosomes), SHUFFLED, with many equal starts,
    start == end intervals, a few long ones (they lift the running maximum of the ends), groups and kinds"""
    chrom, start, end = [], [], []
    for c, n in enumerate(n_per_chrom):
        s = rng.integers(0, span, n)
        s[rng.random(n) < 0.3] = rng.integers(0, span, 1)[0] if n else 0          # ties
        ln = rng.integers(0, max_len, n)
        ln[rng.random(n) < 0.15] = 0                                               # start == end
        ln[rng.random(n) < 0.03] = span                                            # long ones
        chrom.append(np.full(n, c)); start.append(s); end.append(s + ln)
    chrom, start, end = (np.concatenate(x).astype(np.int64) if len(n_per_chrom) else np.zeros(0, np.int64) for x in (chrom, start, end))
    p = rng.permutation(chrom.size)
    chrom, start, end = chrom[p], start[p], end[p]
    return {"chrom": chrom, "start": start, "end": end, "group": rng.integers(0, n_groups, chrom.size), "kind": rng.integers(1, 3, chrom.size)}


def random_queries(rng, n, n_chrom, span=20000, max_len=600, n_groups=7):
    """queries on chromosomes -1 .. n_chrom (the two outer ids exist on the query side only), before / inside / after the subjects' range"""
    s = rng.integers(0, span + 2000, n)
    ln = rng.integers(0, max_len, n)
    ln[rng.random(n) < 0.1] = 0
    ln[rng.random(n) < 0.05] = span
    return {"chrom": rng.integers(-1, n_chrom + 1, n), "start": s, "end": s + ln, "group": rng.integers(0, n_groups, n),
            "kind": rng.integers(1, 3, n)}


def stack(width, qs=1000, qe=2000, n_survive=None, chrom=0):
    """`width` subjects that all lie in the window of the query [qs, qe] and nothing else does: n_survive of them (default all) cover the
    query's middle, the others are single bases at qs (inside the window: start <= qe, end >= qs; ov = 0, never a hit)"""
    n_survive = width if n_survive is None else n_survive
    start = np.concatenate([np.full(n_survive, qs + 10), np.full(width - n_survive, qs)]).astype(np.int64)
    end = np.concatenate([np.full(n_survive, qe - 10), np.full(width - n_survive, qs)]).astype(np.int64)
    return {"chrom": np.full(width, chrom, np.int64), "start": start, "end": end}


def shadowed(width, qs=100000, qe=101000, chrom=0):
    """a wide window with zero survivors: one long subject starts early and ends at qs (a one-base touch: no hit) and lifts the running
    maximum over width - 1 short ones that all end before qs"""
    start = np.concatenate([[10], 20 + 3 * np.arange(width - 1)]).astype(np.int64)
    end = np.concatenate([[qs], start[1:] + 2]).astype(np.int64)
    assert width == 1 or end[1:].max() < qs
    return {"chrom": np.full(width, chrom, np.int64), "start": start, "end": end}


def cases(seed=0):
    """(name, subjects, queries) triples for the host test of the two forms"""
    rng = np.random.default_rng(seed)
    out = []
    for i, per in enumerate(([0], [1], [2], [64, 65], [5, 0, 0, 40], [300, 0, 1, 2, 64])):
        out.append(("random%d" % i, random_set(rng, per), random_queries(rng, 90, len(per))))
    st = stack(70)
    out.append(("stack", st, {"chrom": [0, 0, 0, 1], "start": [1000, 0, 1990, 1000], "end": [2000, 999, 5000, 2000]}))
    sh = shadowed(50)
    out.append(("shadowed", sh, {"chrom": [0, 0], "start": [100000, 5], "end": [101000, 400]}))
    edge = {"chrom": [0, 0, 0, 0], "start": [0, 0, IMAX - 5, IMAX], "end": [0, IMAX, IMAX, IMAX]}
    out.append(("edges", edge, {"chrom": [0, 0, 0, 0], "start": [0, 0, IMAX - 9, IMAX], "end": [IMAX, 7, IMAX, IMAX]}))
    return out
