"""GC content per target on the device (csrc/edgc.inc; gc_content, GcCounter, getBamCounts(reference_fasta=...)) against the plain restatement of
the reference's lines in tests/gc_checker.py.  The counts are integers and are compared exactly; the fractions are gc / atgc in float64 on both
sides and are compared bit for bit, NaN where NaN."""
import ctypes as C
import os

import numpy as np
import pytest

import gc_checker as gck
import readcount_checker as rck

pytestmark = pytest.mark.gpu

WIDTH = 60
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
N_RUN = (3001, 3100)             # bases of "X" that are all N
LOWER_RUN = (3201, 3300)         # ... all lower-case a, c, g, t
IUPAC_RUN = (3401, 3440)         # ... IUPAC codes other than A, C, G, T, N


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """three sequences, 60 bases a line; everything is checked on the third, "X" (9 000 bases), so the two before it are only there to be skipped"""
    rng = np.random.default_rng(20240611)
    x = list(gck.random_sequence(rng, 9000))
    x[N_RUN[0] - 1:N_RUN[1]] = "N" * (N_RUN[1] - N_RUN[0] + 1)
    x[LOWER_RUN[0] - 1:LOWER_RUN[1]] = gck.random_sequence(rng, LOWER_RUN[1] - LOWER_RUN[0] + 1, "acgt")
    x[IUPAC_RUN[0] - 1:IUPAC_RUN[1]] = gck.random_sequence(rng, IUPAC_RUN[1] - IUPAC_RUN[0] + 1, "RYSWKMBDHVryswkmbdhv")
    seqs = {"1": gck.random_sequence(rng, 700), "2": gck.random_sequence(rng, 913, "ACGTN"), "X": "".join(x)}
    data, _ = gck.fasta_bytes([("1 the first", seqs["1"]), ("2", seqs["2"]), ("X last one", seqs["X"])], WIDTH)
    path = str(tmp_path_factory.mktemp("gc") / "genome.fa")
    with open(path, "wb") as f:
        f.write(data)
    from exomedepth_amd.fasta import FastaIndex
    return path, seqs, FastaIndex(path)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                                                            b[~np.isnan(b)].view(np.int64))


def _check(ed, genome, chrom, start, end, **kw):
    path, seqs, idx = genome
    flank = kw.get("flank", 0)
    ws, we = gck.widened(seqs, chrom, start, end, flank) if flank else (start, end)
    want_gc, want_atgc = gck.gc_counts(seqs, chrom, ws, we)
    gc, atgc = ed.gc_content(idx, chrom, start, end, counts=True, **kw)
    assert gc.dtype == np.int32 and atgc.dtype == np.int32
    assert np.array_equal(gc, want_gc) and np.array_equal(atgc, want_atgc)
    frac = ed.gc_content(path, chrom, start, end, **kw)
    assert _same_bits(frac, gck.gc_fraction(seqs, chrom, ws, we))
    return gc, atgc, frac


def test_range_edges(edlib, genome):
    path, seqs, idx = genome
    S = edlib.gc_geometry()["segment_bytes"]
    assert edlib.gc_geometry() == {"block": 256, "segment_bytes": S, "step_bytes": 1024, "lane_bytes": 16} and S % 1024 == 0 and 2 * S + 1 + 80 < 9000
    n = len(seqs["X"])
    lengths = LENGTHS + [S - 1, S, S + 1, 2 * S + 1]
    start, end = [], []
    for L in lengths:
        for s in range(100, 118):                     # 18 neighbouring starts: every residue of the byte address modulo 16 (asserted below)
            start.append(s); end.append(s + L - 1)
        start += [1, n - L + 1]                       # touching the first and the last base of the sequence
        end += [L, n]
        for line in (3, 40):                          # ending exactly on a line end, and beginning right after one
            start += [line * WIDTH - L + 1 if line * WIDTH >= L else 1, line * WIDTH + 1]
            end += [line * WIDTH, line * WIDTH + L]
    # the segment is a length in BYTES: ranges whose byte length is S - 1, S, S + 1 and 2 S + 1, from every one of the 18 starts
    for s in range(100, 118):
        e = np.arange(s, n + 1)
        first, last = idx.byte_range("X", np.full(e.size, s), e)
        for want in (S - 1, S, S + 1, 2 * S + 1):
            hit = np.flatnonzero(last - first == want)           # none where that byte is a line end
            if hit.size:
                start.append(s); end.append(int(e[hit[0]]))
    start, end = np.asarray(start), np.asarray(end)
    chrom = ["X"] * start.size
    first, last = idx.byte_range(chrom, start, end)
    assert set(((first - first.min()) % 16).tolist()) == set(range(16)) == set((first % 16).tolist())
    for L in lengths:
        assert set((first[(end - start + 1 == L)] % 16).tolist()) == set(range(16))
    assert {S - 1, S, S + 1, 2 * S + 1} <= set((last - first).tolist())
    assert np.any(end % WIDTH == 0) and np.any(start % WIDTH == 1) and start.min() == 1 and end.max() == n
    gc, atgc, _ = _check(edlib, genome, chrom, start, end)
    assert atgc.max() > S // 2 and gc.min() == 0                 # (half the alphabet is A, C, G, T) and a one-base target need not be G or C


def test_letters(edlib, genome):
    path, seqs, idx = genome
    chrom = ["X"] * 5
    start = [N_RUN[0], LOWER_RUN[0], IUPAC_RUN[0], N_RUN[0] - 1, LOWER_RUN[0]]
    end = [N_RUN[1], LOWER_RUN[1], IUPAC_RUN[1], N_RUN[1] + 1, LOWER_RUN[0]]
    gc, atgc, frac = _check(edlib, genome, chrom, start, end)
    assert atgc[0] == 0 and np.isnan(frac[0])                    # all N: no letter to count, NA
    assert atgc[1] == LOWER_RUN[1] - LOWER_RUN[0] + 1 and 0 < gc[1] < atgc[1]          # lower case counts as upper case
    assert atgc[2] == 0 and np.isnan(frac[2])                    # S is "G or C" to a biologist and no letter here, like the rest
    assert atgc[3] <= 2 and atgc[4] == 1


def _cuts_layout(idx, n, batch):
    """a first target whose first byte puts a cut of the pieces (its address + k * batch) on a base, and targets placed on the cuts"""
    addr = idx.byte_range("X", np.arange(1, n + 1), np.arange(1, n + 1))[0]
    base_at = {int(a): k + 1 for k, a in enumerate(addr)}
    for s0 in range(1, 200):
        a = int(addr[s0 - 1])
        if a + batch in base_at and a + 2 * batch in base_at and a + 2 * batch - 1 in base_at:
            break
    else:
        raise AssertionError("no such first target")
    c1, c2 = base_at[a + batch], base_at[a + 2 * batch]          # the bases at the first and the second cut (c2 not the first of its line)
    start = [s0, c1 - 30, c1, c1 - 10, c2 - 1, s0 + 5, c1 + 1, c2]
    end = [s0 + 9, c1 + 30, c1 + 40, c2 + 10, c2, c2 + 100, c2 - 1, n]
    return a, np.asarray(start), np.asarray(end)


def test_chunk_independence(edlib, genome):
    path, seqs, idx = genome
    n = len(seqs["X"])
    a, start, end = _cuts_layout(idx, n, 4096)
    rng = np.random.default_rng(5)
    rs = rng.integers(start[0], n - 400, 150)
    start = np.concatenate([start, rs]); end = np.concatenate([end, rs + rng.integers(0, 400, 150)])
    chrom = ["X"] * start.size
    first, last = idx.byte_range(chrom, start, end)
    assert first.min() == a == first[0]
    cuts = a + 4096 * np.arange(1, 3)
    assert last.max() > cuts[1]                                              # three pieces
    assert np.any((first < cuts[0]) & (last > cuts[0]) & (last <= cuts[1]))  # a target astride one cut
    assert np.any((first < cuts[0]) & (last > cuts[1]))                      # a target in three pieces
    assert np.any(first == cuts[0]) and np.any(first == cuts[1])             # targets that begin exactly at a cut
    assert np.any(last == cuts[1])                                           # ... and one that ends exactly there
    got = {b: edlib.gc_content(idx, chrom, start, end, counts=True, batch_bytes=b) for b in (4096, 4097, 64 << 20, 1000, 17)}
    want = gck.gc_counts(seqs, chrom, start, end)
    for b, (gc, atgc) in got.items():
        assert np.array_equal(gc, want[0]) and np.array_equal(atgc, want[1]), b
    assert _same_bits(edlib.gc_content(path, chrom, start, end, batch_bytes=4096), edlib.gc_content(path, chrom, start, end))


def test_order_duplicates_and_sequences(edlib, genome):
    path, seqs, idx = genome
    rng = np.random.default_rng(9)
    m = 120
    chrom = np.asarray(["1", "2", "X"], dtype=object)[rng.integers(0, 3, m)]
    length = np.asarray([len(seqs[c]) for c in chrom])
    start = (rng.random(m) * (length - 1)).astype(np.int64) + 1
    end = np.minimum(start + rng.integers(0, 300, m), length)
    gc, atgc, frac = _check(edlib, genome, list(chrom), start, end)
    perm = rng.permutation(m)
    g2, a2, f2 = _check(edlib, genome, list(chrom[perm]), start[perm], end[perm])
    assert np.array_equal(g2, gc[perm]) and np.array_equal(a2, atgc[perm]) and _same_bits(f2, frac[perm])
    twice = np.concatenate([np.arange(m), [7, 7, 0]])                        # a target listed again has its value again
    g3, a3, _ = _check(edlib, genome, list(chrom[twice]), start[twice], end[twice], batch_bytes=1024)
    assert np.array_equal(g3, gc[twice]) and g3[-2] == g3[-3] == gc[7]
    only = np.flatnonzero(chrom == "X")                                       # the third sequence only: the two before it are not read
    g4, _, _ = _check(edlib, genome, ["X"] * only.size, start[only], end[only])
    assert np.array_equal(g4, gc[only])
    gc0, atgc0 = edlib.gc_content(idx, [], [], [], counts=True)
    assert gc0.shape == atgc0.shape == (0,) and gc0.dtype == np.int32
    assert edlib.gc_content(path, [], [], []).shape == (0,)
    for bad in ((["Y"], [1], [2], "not in"), (["1"], [1], [701], "beyond the 700 bases"), (["1"], [0], [5], "1 <= start"), (["1"], [5], [4], "1 <= start")):
        with pytest.raises(ValueError, match=bad[3]):
            edlib.gc_content(idx, *bad[:3])


def test_flank(edlib, genome):
    path, seqs, idx = genome
    chrom = ["1", "1", "1", "X", "X", "2"]
    start = [1, 30, 690, 8990, 4000, 400]
    end = [10, 40, 700, 9000, 4100, 420]
    plain = _check(edlib, genome, chrom, start, end)
    for flank in (25, 50, 10000):                                # 25 clips at the ends only; 10 000 makes every target its whole sequence
        gc, atgc, _ = _check(edlib, genome, chrom, start, end, flank=flank)
        assert np.all(atgc >= plain[1])
    whole = gck.gc_counts(seqs, ["1", "X", "2"], [1, 1, 1], [700, 9000, 913])
    assert gc[0] == gc[1] == gc[2] == whole[0][0] and gc[3] == gc[4] == whole[0][1] and gc[5] == whole[0][2]


def test_add_refusals_and_pieces(edlib, genome):
    """ed_gc_add through ctypes: what it refuses, what it accepts, and ranges that reach beyond the piece on both sides or miss it"""
    from exomedepth_amd import EdError, _lib
    L = _lib.lib()
    data = np.frombuffer(b"ACGTNNacgtGGGG\nCCAT" * 300, dtype=np.uint8)
    n = data.size
    h = C.c_void_p()
    assert L.ed_gc_create(C.byref(h), 0, 3) == 0

    def add(buf, n_bytes, off, first, last, target, n_ranges=None):
        a = [np.asarray(v, dtype=np.int64) for v in (first, last, target)]
        p = [v.ctypes.data_as(C.c_void_p) if v.size else None for v in a]
        return L.ed_gc_add(h, buf.ctypes.data_as(C.c_void_p) if buf is not None else None, n_bytes, off, a[0].size if n_ranges is None else n_ranges, *p)

    for first, last, target, msg in (([0], [5], [3], b"target 3 outside 0 .. 2"), ([0], [5], [-1], b"target -1 outside"), ([0, 6], [5, 5], [0, 1], b"range 1 is [6, 5)")):
        assert add(data, n, 0, first, last, target) == -1 and msg in L.ed_last_error()
    assert add(data, -1, 0, [0], [5], [0]) == -1 and add(data, n, -4, [0], [5], [0]) == -1 and add(data, n, 0, [0], [5], [0], n_ranges=-1) == -1
    assert add(None, n, 0, [0], [5], [0]) == -1 and L.ed_gc_add(h, data.ctypes.data_as(C.c_void_p), n, 0, 1, None, None, None) == -1
    assert L.ed_gc_create(C.byref(C.c_void_p()), 0, -1) == -1
    gc, atgc = np.full(3, -1, np.int32), np.full(3, -1, np.int32)
    out = [v.ctypes.data_as(C.c_void_p) for v in (gc, atgc)]
    assert L.ed_gc_copy(h, *out) == 0 and not gc.any() and not atgc.any()    # nothing a refused call was given has been counted
    assert add(data, n, 0, [], [], []) == 0 and add(None, 0, 0, [], [], []) == 0 and add(None, 0, 77, [0], [5], [0]) == 0
    assert add(data, n, 0, [5], [5], [2]) == 0                               # an empty range
    # target 0: the whole file and more, given piece by piece with the same range; target 1: a range inside the second piece; target 2: misses
    cut = [0, 1000, 1001, 3333, n]
    for a, b in zip(cut[:-1], cut[1:]):
        assert add(data[a:b].copy(), b - a, 10**12 + a, [10**12 - 50, 10**12 + 1003, 5], [10**12 + n + 50, 10**12 + 1200, 10**12], [0, 1, 2]) == 0
    assert L.ed_gc_copy(h, *out) == 0
    text = data.tobytes().upper()
    count = lambda x: (x.count(b"G") + x.count(b"C"), sum(x.count(c) for c in (b"A", b"C", b"G", b"T")))
    assert (gc[0], atgc[0]) == count(text) and (gc[1], atgc[1]) == count(text[1003:1200]) and (gc[2], atgc[2]) == (0, 0)
    ms = C.c_double(-1)
    assert L.ed_gc_kernel_ms(h, C.byref(ms)) == 0 and ms.value > 0 and L.ed_gc_kernel_ms(h, None) == -1
    L.ed_gc_destroy(h)
    L.ed_gc_destroy(None)
    c = edlib.GcCounter(2)
    c.close()
    with pytest.raises(EdError, match="closed"):
        c.counts()


def test_getBamCounts_gains_the_column(edlib, genome, tmp_path):
    path, seqs, idx = genome
    rng = np.random.default_rng(77)
    refs = [("X", 9000), ("1", 700), ("2", 913)]
    bams = []
    for k in range(2):
        m = 6000
        refid = rng.integers(0, 3, m)
        pos = (rng.random(m) * np.asarray([8800, 600, 800])[refid]).astype(int)
        recs = [(int(r), int(p), 60, 0x1 | 0x2, 100) for r, p in zip(refid, pos)]
        bams.append(str(tmp_path / ("sample%d.bam" % k)))
        rck.write_bam(bams[-1], "@HD\tVN:1.6\n", refs, recs)
    # BED rows (0-based start), out of order, with names; none inside the runs without letters
    bstart = np.concatenate([np.arange(0, 2900, 100), np.arange(3500, 8900, 100), [0, 300], [100, 500]])
    chrom = ["X"] * (29 + 54) + ["1", "1", "2", "2"]
    perm = rng.permutation(bstart.size)
    frame = {"chromosome": [chrom[i] for i in perm], "start": bstart[perm], "end": bstart[perm] + 100,
             "name": np.asarray(["e%d" % i for i in perm], dtype=object)}
    plain = edlib.getBamCounts(bed_frame=frame, bam_files=bams)
    out = edlib.getBamCounts(bed_frame=frame, bam_files=bams, reference_fasta=path)
    assert list(plain.keys()) == ["chromosome", "start", "end", "exon", "sample0.bam", "sample1.bam"]
    assert list(out.keys()) == ["chromosome", "start", "end", "exon", "GC", "sample0.bam", "sample1.bam"]
    for k in plain:
        assert np.array_equal(np.asarray(out[k]), np.asarray(plain[k])), k
    assert list(out["chromosome"][:4]) == ["1", "1", "2", "2"]                 # the re-ordered rows: '1' .. '22' first
    assert _same_bits(out["GC"], gck.gc_fraction(seqs, out["chromosome"], out["start"], out["end"]))
    assert not np.isnan(out["GC"]).any() and out["GC"].std() > 0
    # without a name column GC comes right after `end`; a FastaIndex serves as well as a path
    bare = edlib.getBamCounts(bed_frame={k: frame[k] for k in ("chromosome", "start", "end")}, bam_files=bams[:1], reference_fasta=idx)
    assert list(bare.keys()) == ["chromosome", "start", "end", "GC", "sample0.bam"] and _same_bits(bare["GC"], out["GC"])
    # a bad FASTA fails before any BAM file is opened
    with pytest.raises(ValueError, match="beyond the 700 bases"):
        edlib.getBamCounts(bed_frame={"chromosome": ["1"], "start": [650], "end": [750]}, bam_files=[str(tmp_path / "no_such.bam")], reference_fasta=path)
    # the column is what the covariate model takes
    test, ref = out["sample0.bam"], out["sample1.bam"]
    assert np.sum(test > 5) >= 5
    x = edlib.ExomeDepth(test, ref, data={"GC": out["GC"]}, formula="cbind(test, reference) ~ GC")
    assert x.expected.shape == (test.size,) and np.all((x.expected > 0) & (x.expected < 1)) and x.likelihood.shape == (test.size, 3)
    assert np.isfinite(x.likelihood).all()
