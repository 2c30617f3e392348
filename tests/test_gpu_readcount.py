"""Reads per exon on the device (csrc/edreadcount.inc; ReadCounter, getBamCounts, count_everted_reads) against the brute-force statement of
the two R functions in tests/readcount_checker.py.  Counts are integers: every comparison is exact equality."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import readcount_checker as rck

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "minimum_1_25630000_25650000.bam")
PAIR = 0x1 | 0x2                        # a record getBamCounts takes: paired, proper pair
EVERTED = 0x1 | 0x10                    # a record the everted rule takes with tlen > 0: paired, not proper, reverse strand


def _rec(refid, pos, tlen, flag, mapq):
    """four record arrays from per-record values (scalars are broadcast)"""
    refid, pos, tlen, flag, mapq = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (refid, pos, tlen, flag, mapq)))
    return (refid.astype(np.int32).ravel(), pos.astype(np.int32).ravel(), tlen.astype(np.int32).ravel(),
            (flag | (mapq << 16)).astype(np.uint32).ravel())


def _cat(*recs):
    return tuple(np.concatenate([r[k] for r in recs]) for k in range(4))


def _take(rec, idx):
    return tuple(a[idx] for a in rec)


def _device(ed, chrom, start, end, rec, ref_names, mode, min_mapq=20, read_width=300, chunks=None):
    rc = ed.ReadCounter(chrom, start, end, 1)
    try:
        for part in ([rec] if chunks is None else chunks):
            rc.add(0, part, ref_names, mode=mode, min_mapq=min_mapq, read_width=read_width)
        rc.finish(0)
        return rc.counts()[:, 0].astype(np.int64)
    finally:
        rc.close()


def _check(ed, chrom, start, end, rec, ref_names, mode, min_mapq=20, read_width=300):
    """device == checker, exactly; returns the counts"""
    levels = list(dict.fromkeys(str(c) for c in chrom))
    ids = np.asarray([levels.index(str(c)) for c in chrom])
    r2c = np.asarray([levels.index(r) if r in levels else -1 for r in ref_names])
    want = rck.ref_counts(mode, ids, start, end, rec, r2c, min_mapq, read_width)
    got = _device(ed, chrom, start, end, rec, ref_names, mode, min_mapq, read_width)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])
    return got


# the twelve exons of the edge tests: nested, duplicated, equal starts, equal ends, one of length 1, two abutting
EX_S = np.array([100, 120, 120, 100, 100, 150, 300, 400, 451, 600, 600, 700])
EX_E = np.array([200, 180, 180, 160, 250, 250, 300, 450, 500, 650, 650, 800])


def test_interval_edges(edlib):
    fs, fe = [], []
    for s, e in zip(EX_S, EX_E):
        fs += [e, e + 1, s - 30, s - 31]             # frag.start == exon.end / == exon.end + 1; frag.end == exon.start / == exon.start - 1
        fe += [e + 30, e + 31, s, s - 1]
    fs += [50, 10, 900]                              # one covers every exon, one lies before the first, one after the last
    fe += [1000, 60, 950]
    fs, fe = np.asarray(fs), np.asarray(fe)
    rec = _rec(0, fs - 1, fe - fs, PAIR, 40)         # mode 0: [pos + 1, pos + 1 + tlen]
    got = _check(edlib, ["7"] * 12, EX_S, EX_E, rec, ["7"], 0)
    assert got.min() >= 2 and got[1] == got[2] and got[9] == got[10]          # every exon: its own edge fragments + the covering one; duplicates agree
    ev = _rec(0, fe - 1, fs - fe, 0x1, 40)           # mode 1, forward strand, tlen < 0: [pos + 1 + tlen, pos + 1]
    assert np.array_equal(_check(edlib, ["7"] * 12, EX_S, EX_E, ev, ["7"], 1), got)
    ev = _rec(0, fs - 1, fe - fs, EVERTED, 40)       # reverse strand, tlen > 0
    assert np.array_equal(_check(edlib, ["7"] * 12, EX_S, EX_E, ev, ["7"], 1), got)


def test_filters(edlib):
    """every filter bit flipped one at a time from a record that passes, times every tlen and mapq of interest, for both modes.  Every record
    has an exon of its own that holds its fragment whatever its tlen, so the count vector says record by record who was taken"""
    bits = [0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800]
    tlens = (0, -1, 1, 150, -150, 99999, -99999, 100000, -100000)
    mapqs = (0, 19, 20, 21, 35, 254, 255)
    for mode, base in ((0, PAIR), (0, 0), (1, EVERTED), (1, 0x1)):
        flags = [base] + [base ^ b for b in bits]
        f, t, q = (a.ravel() for a in np.meshgrid(flags, tlens, mapqs, indexing="ij"))
        k = np.arange(f.size)
        start, end = 300000 * k + 1, 300000 * k + 250000
        rec = _rec(0, 300000 * k + 120000, t, f, q)
        plain = int(np.flatnonzero((f == base) & (t == (-150 if base == 0x1 else 150)) & (q == 35))[0])
        for rw in (0, 300):
            got = _check(edlib, ["1"] * k.size, start, end, rec, ["1"], mode, 20, rw)
            assert got.max() == 1 and got[plain] == 1 and 0 < got.sum() < k.size       # the unflipped record is counted, and not everything is
    # mapq == min_mapq: out under getBamCounts' rule, in under the everted one; 255 out in both
    for mode, flag, want in ((0, PAIR, [0, 1, 0]), (1, EVERTED, [1, 1, 0])):
        got = [_check(edlib, ["1"], [1], [5000], _rec(0, 100, 150, flag, q), ["1"], mode, 20)[0] for q in (20, 21, 255)]
        assert got == want
    # refID -1, a refID beyond the header, a reference that is no target
    rec = _rec([-1, 5, 1, 0, 2], 100, 150, PAIR, 40)
    assert _check(edlib, ["b", "a"], [1, 1], [5000, 5000], rec, ["a", "zz", "b"], 0).tolist() == [1, 1]
    # unpaired reads: read_width 0 is the single base pos + 1
    rec = _rec(0, [99, 100, 101, 199, 200], 0, 0, 40)
    assert _check(edlib, ["1"], [101], [200], rec, ["1"], 0, 20, 0).tolist() == [3]
    assert _check(edlib, ["1"], [101], [200], rec, ["1"], 0, 20, 300).tolist() == [4]


def test_chromosomes(edlib):
    """three target chromosomes -- one whose exons no fragment hits, one without records, one with a single exon -- and a header whose order is
    not the targets' (ref_to_chrom is not the identity)"""
    chrom = ["B"] * 4 + ["A"] * 3 + ["C"]
    start = [100, 300, 500, 700, 100, 200, 300, 1000]
    end = [200, 400, 600, 800, 150, 250, 350, 2000]
    ref_names = ["x0", "C", "A", "x1", "B"]
    rng = np.random.default_rng(5)
    n = 500
    on_b = _rec(4, rng.integers(5000, 9000, n), rng.integers(1, 300, n), PAIR, 40)       # B: records, none near its exons
    on_c = _rec(1, rng.integers(500, 2500, n), rng.integers(1, 300, n), PAIR, 40)
    off = _rec(rng.choice([0, 3], n), rng.integers(0, 1000, n), 200, PAIR, 40)
    got = _check(edlib, chrom, start, end, _cat(on_b, on_c, off), ref_names, 0)
    assert got[:7].sum() == 0 and got[7] > 0


def test_geometry(edlib):
    """record counts on the launch geometry's edges; a whole wave of equal ranks; ranks alternating lane by lane"""
    g = edlib.readcount_geometry()
    per = g["records_per_workgroup"]
    assert g["block"] % 64 == 0 and per % g["block"] == 0
    rng = np.random.default_rng(11)
    E = 300
    start = 1000 + 500 * np.arange(E)
    end = start + rng.integers(50, 700, E)                                    # neighbours overlap now and then
    chrom = ["1"] * E
    big = 3 * per + 7
    pos = np.sort(rng.integers(0, 1000 + 500 * E + 2000, big))
    rec = _rec(0, pos, rng.integers(1, 600, big), PAIR, 40)
    for n in (0, 1, 63, 64, 65, per - 1, per, per + 1, big):
        _check(edlib, chrom, start, end, _take(rec, slice(0, n)), ["1"], 0)
    one_bin = _rec(0, 1000 + 500 * 7 + 10, 20, PAIR, 40)                      # 20 000 records on one exon: every add is a merged run of 64
    one_bin = tuple(np.repeat(a, 20000) for a in one_bin)
    got = _check(edlib, chrom, start, end, one_bin, ["1"], 0)
    assert got[7] == 20000
    alt = _rec(0, np.where(np.arange(20001) % 2 == 0, 1000 + 500 * 3 + 10, 1000 + 500 * 200 + 10), 20, PAIR, 40)   # no run longer than 1
    got = _check(edlib, chrom, start, end, alt, ["1"], 0)
    assert got[3] == 10001 and got[200] == 10000


def test_finish_scan_crosses_its_block(edlib):
    """a chromosome of more exons than one step of the finish scan (and one of exactly a step), so the carry is used"""
    g = edlib.readcount_geometry()
    F = g["finish_block"]
    rng = np.random.default_rng(13)
    sizes = (2 * F + 37, F, 1)
    chrom = sum((["c%d" % i] * n for i, n in enumerate(sizes)), [])
    start = np.concatenate([100 + 40 * np.arange(n) for n in sizes])
    end = start + rng.integers(0, 90, start.size)
    n = 30000
    rec = _rec(rng.integers(0, 3, n), rng.integers(0, 40 * (2 * F + 60), n), rng.integers(1, 400, n), PAIR, 40)
    _check(edlib, chrom, start, end, rec, ["c0", "c1", "c2"], 0)


def _mixed(rng, n, n_ref, span):
    """records in a mix of everything: both kinds of pair, unpaired, all flag bits, all mapq, both signs of tlen, refID -1 and beyond"""
    flag = rng.integers(0, 4096, n)
    flag = np.where(rng.random(n) < 0.35, PAIR | (flag & 0x30), flag)
    flag = np.where(rng.random(n) < 0.2, 0x1 | (flag & 0x30), flag)
    mapq = rng.choice([0, 19, 20, 21, 40, 60, 255], n)
    tlen = np.where(rng.random(n) < 0.9, rng.integers(-600, 600, n), rng.choice([0, 99999, 100000, -99999, -100000], n))
    return _rec(rng.integers(-1, n_ref + 1, n), rng.integers(0, span, n), tlen, flag, mapq)


@pytest.fixture(scope="module")
def design():
    """2 000 exons over 5 chromosomes, 20 % of them overlapping their predecessor"""
    rng = np.random.default_rng(17)
    sizes = (700, 500, 400, 399, 1)
    chrom, start, end = [], [], []
    for c, n in enumerate(sizes):
        gap = rng.integers(50, 3000, n)
        width = rng.integers(1, 900, n)
        s = 1000 + np.cumsum(gap + width)
        over = rng.random(n) < 0.2
        s = np.where(over, np.maximum(1, s - gap - rng.integers(1, 200, n)), s)      # reaches back into the exon before
        chrom += ["k%d" % c] * n
        start.append(s); end.append(s + width)
    start, end = np.concatenate(start), np.concatenate(end)
    perm = rng.permutation(start.size)                                               # exons in no particular order
    return [chrom[i] for i in perm], start[perm], end[perm], ["k3", "u", "k0", "k4", "k1", "k2"], int(end.max()) + 2000


@pytest.mark.parametrize("mode", [0, 1])
def test_randomised(edlib, design, mode):
    chrom, start, end, ref_names, span = design
    rec = _mixed(np.random.default_rng(100 + mode), 200000, len(ref_names), span)
    got = _check(edlib, chrom, start, end, rec, ref_names, mode)
    assert got.sum() > 1000


def test_chunking_and_order(edlib, design):
    chrom, start, end, ref_names, span = design
    rng = np.random.default_rng(23)
    rec = _mixed(rng, 30000, len(ref_names), span)
    rec = _take(rec, np.argsort(rec[0].astype(np.int64) * 2**32 + rec[1], kind="stable"))      # coordinate-sorted, as a BAM is
    whole = _check(edlib, chrom, start, end, rec, ref_names, 0)
    cuts = [0, 1, 64, 1000, 1001, 9000, 20001, 30000]
    ragged = _device(edlib, chrom, start, end, rec, ref_names, 0, chunks=[_take(rec, slice(a, b)) for a, b in zip(cuts[:-1], cuts[1:])])
    shuffled = _device(edlib, chrom, start, end, _take(rec, rng.permutation(30000)), ref_names, 0)
    assert np.array_equal(ragged, whole) and np.array_equal(shuffled, whole)
    rc = edlib.ReadCounter(chrom, start, end, 1)                                               # two add / finish rounds accumulate
    for part in (_take(rec, slice(0, 12345)), _take(rec, slice(12345, 30000))):
        rc.add(0, part, ref_names)
        rc.finish(0)
    rc.finish(0)                                                                               # nothing added: nothing changes
    assert np.array_equal(rc.counts()[:, 0], whole)
    rc.close()


def test_columns(edlib, design):
    from exomedepth_amd import EdError, _lib
    chrom, start, end, ref_names, span = design
    levels = list(dict.fromkeys(chrom))
    ids = np.asarray([levels.index(c) for c in chrom])
    r2c = np.asarray([levels.index(r) if r in levels else -1 for r in ref_names])
    rc = edlib.ReadCounter(chrom, start, end, 4)
    recs = [_mixed(np.random.default_rng(40 + k), 5000 + 3000 * k, len(ref_names), span) for k in range(4)]
    modes = (0, 1, 0, 0)
    for k in (2, 0, 3, 1):                                                   # in no particular order
        rc.add(k, recs[k], ref_names, mode=modes[k])
        if k == 3:
            with pytest.raises(EdError, match="status -5"):                  # a copy before finish: ED_ERR_STATE
                rc.counts()
            with pytest.raises(EdError, match="status -5"):
                rc.counts(3, 1)
            with pytest.raises(EdError, match="status -5"):
                rc.device_counts(exon_major=True)
            with pytest.raises(EdError, match="status -5"):                  # another column before finish
                rc.add(1, recs[1], ref_names)
            assert rc.counts(0, 3).shape == (len(chrom), 3)                  # columns that are not pending can be read
        rc.finish(k)
    whole = rc.counts()
    assert whole.shape == (len(chrom), 4) and whole.dtype == np.int32
    for k in range(4):
        assert np.array_equal(whole[:, k], rck.ref_counts(modes[k], ids, start, end, recs[k], r2c))
    assert np.array_equal(rc.counts(1, 2), whole[:, 1:3]) and np.array_equal(rc.counts(3), whole[:, 3:])
    assert np.array_equal(rc.device_counts().to_host(), whole.T)
    em = rc.device_counts(exon_major=True)                                   # 2 000 x 4: tiles cut on both sides
    assert np.array_equal(em.to_host(), whole)
    em.free()
    L, h = _lib.lib(), rc.handle
    four = [np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)] * 4
    for bad in ((-1, 0, 300), (4, 0, 300), (0, 2, 300), (0, -1, 300), (0, 0, -1)):            # column, mode, read_width
        assert L.ed_readcount_add(h, bad[0], bad[1], 1, *four, 1, four[0], 20, bad[2]) == -1
    assert L.ed_readcount_add(h, 0, 0, 1, *four, 1, np.array([5], np.int32).ctypes.data_as(C.c_void_p), 20, 300) == -1
    assert L.ed_readcount_add(h, 0, 0, 0, None, None, None, None, 0, None, 20, 300) == 0     # no records: valid
    assert L.ed_readcount_finish(h, 4) == -1 and L.ed_readcount_copy(h, 3, 2, four[0]) == -1
    assert np.array_equal(rc.counts(), whole)
    rc.close()
    with pytest.raises(EdError, match="1 <= start <= end"):
        edlib.ReadCounter(["1"], [5], [4], 1)


def _tiles():
    s = np.arange(25630000, 25650000, 200)
    chrom = ["1"] * s.size + ["1"] * 3
    start = np.concatenate([s, [25630000, 25635000, 25635100]])             # BED: 0-based start, closed end
    end = np.concatenate([s + 200, [25650000, 25645000, 25636000]])
    name = np.asarray(["t%d" % i for i in range(start.size)], dtype=object)
    perm = np.random.default_rng(3).permutation(start.size)
    return {"chromosome": [chrom[i] for i in perm], "start": start[perm], "end": end[perm], "name": name[perm]}


def test_fixture_end_to_end(edlib, tmp_path):
    slow = rck.parse_bam(FIXTURE)
    frame = _tiles()
    out = edlib.getBamCounts(bed_frame=frame, bam_files=[FIXTURE])
    base = os.path.basename(FIXTURE)
    assert list(out.keys()) == ["chromosome", "start", "end", "exon", base]
    t = edlib.bed_targets(bed_frame=frame)
    r2c = np.asarray([0 if r == "1" else -1 for r in slow["ref_names"]])
    want = rck.ref_counts(0, np.zeros(t["start"].size, int), t["start"], t["end"], slow["records"], r2c, 20, 300)
    assert np.array_equal(out[base], want) and out[base].sum() > 0
    assert np.array_equal(out["start"], t["start"]) and list(out["exon"]) == list(t["exon"])
    spans = {"chromosome": ["1", "1"], "start": [2580000, 2610000], "end": [2610000, 2640000]}      # where the file's everted pairs lie
    ev = {}
    for q in (0, 35):
        ev[q] = edlib.count_everted_reads(bed_frame=spans, bam_files=[FIXTURE], min_mapq=q)[base]
        assert np.array_equal(ev[q], rck.ref_counts(1, [0, 0], np.asarray(spans["start"]) + 1, spans["end"], slow["records"], r2c, q))
    assert ev[0].sum() >= ev[35].sum() >= 1
    # the same file rewritten in 300-byte blocks (records straddle nearly every block), and under another name: a second column
    raw = open(FIXTURE, "rb").read()
    import zlib
    stream, off = bytearray(), 0
    while off < len(raw):
        d = zlib.decompressobj(31)
        stream += d.decompress(raw[off:])
        off = len(raw) - len(d.unused_data)
    small = str(tmp_path / "rewritten.bam")
    rck.write_bgzf(small, bytes(stream), 300)
    two = edlib.getBamCounts(bed_frame=frame, bam_files=[FIXTURE, small])
    assert list(two.keys())[-2:] == [base, "rewritten.bam"]
    assert np.array_equal(two[base], want) and np.array_equal(two["rewritten.bam"], want)


def _live():
    from exomedepth_amd import _lib
    n, by = C.c_int64(-1), C.c_int64(-1)
    _lib.lib().ed_live_allocations(C.byref(n), C.byref(by))
    return n.value, by.value


def test_resident_matrix_feeds_the_cohort(edlib):
    """the device matrix of a 6-sample run goes to Cohort.submit as it lies (sample-major, counts_layout 1), and its exon-major transpose to
    correct_counts_using_PCA, no host copy; the results equal what the host copies of the same matrix give; the owners' counters come back to
    where they were"""
    from exomedepth_amd import _lib, synth
    ed = edlib
    gc.collect()
    assert _lib.lib().ed_release_scratch() == 0
    _lib.lib().ed_dropin_release()
    live0 = _live()
    E, S = 600, 6
    chrom_off, start, end = synth.exon_design(E, 2, seed=5)
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    chrom = np.repeat(["1", "2"], np.diff(chrom_off))
    rc = ed.ReadCounter(chrom, start, end, S)
    rng = np.random.default_rng(29)
    fa, fb = np.linspace(-1, 1, S), np.cos(np.arange(S))                     # two factors across the samples, so the PCA below has something to find
    for s in range(S):
        n = 60000 + 5000 * s
        w = 1 + 0.6 * fa[s] * np.sin(np.arange(E) / 40.0) + 0.35 * fb[s] * np.cos(np.arange(E) / 17.0)
        e = rng.choice(E, n, p=w / w.sum())
        pos = start[e] + rng.integers(-150, 100, n)
        rec = _rec(np.where(e < chrom_off[1], 0, 1), np.maximum(pos, 0), rng.integers(100, 300, n), PAIR, 40)
        rc.add(s, rec, ["1", "2"])
        rc.finish(s)
    assert _live()[0] > live0[0]
    dev = rc.device_counts()
    host = dev.to_host()                                                     # (S, E)
    assert host.shape == (S, E) and np.array_equal(host.T, rc.counts()) and host.min() >= 0 and np.median(host) > 20
    ref_host = np.ascontiguousarray(np.roll(host, 1, axis=0) + np.roll(host, 2, axis=0))
    results = []
    for test in (dev, host):
        plan = ed.Plan(chrom_off, start, end)
        co = ed.Cohort(plan, S, 2, emit_mode=2, counts_layout=1)
        t = co.submit(test, ref_host, n_samples=S)
        results.append(co.results(t, S, path=True))
        co.close(); plan.close()
    a, b = results
    assert np.array_equal(a["calls"], b["calls"]) and np.array_equal(a["path"], b["path"])
    assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["expected"], b["expected"])
    for k in a["info"].dtype.names:
        assert np.array_equal(a["info"][k], b["info"][k])
    # the exon-major form, transposed on the device, to correct_counts_using_PCA: the same corrected matrix as from the host copy
    em = rc.device_counts(exon_major=True)
    assert em.shape == (E, S) and np.array_equal(em.to_host(), host.T)
    pca = [ed.correct_counts_using_PCA(x, nPCs=2) for x in (em, np.ascontiguousarray(host.T))]
    assert np.array_equal(pca[0].to_host(), pca[1].to_host()) and not np.array_equal(pca[0].to_host(), host.T)
    for x in pca + [em]:
        x.free()
    del dev, test, em, pca
    rc.close()
    gc.collect()
    assert _lib.lib().ed_release_scratch() == 0
    assert _live() == live0
