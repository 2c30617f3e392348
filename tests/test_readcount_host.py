"""The host side of the read counter: BGZF blocks -> record stream -> record fields (exomedepth_amd/bam.py + ed_bam_scan_records), and the
target frame of getBamCounts / count.everted.reads.  No device is needed; the other side of every comparison is tests/readcount_checker.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import readcount_checker as rck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "minimum_1_25630000_25650000.bam")
REFS = [("1", 249250621), ("2", 243199373), ("MT", 16569)]
TEXT = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:1\tLN:249250621\n"


def _records(n=57, seed=3):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(-1, 3)), int(rng.integers(0, 10**6)), int(rng.integers(0, 61)), int(rng.integers(0, 4096)),
             int(rng.integers(-500, 500))) for _ in range(n)]


def _expected(records):
    a = np.asarray([(r[0], r[1], r[4], r[3] | (r[2] << 16)) for r in records], dtype=np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.uint32)


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.fixture(scope="module")
def small():
    recs = _records()
    stream, first = rck.bam_stream(TEXT, REFS, recs)
    return recs, stream, first


def _boundaries(stream, first):
    out, p = [first], first
    while p < len(stream):
        p += 4 + struct.unpack_from("<i", stream, p)[0]
        out.append(p)
    assert p == len(stream)
    return out


def _payloads(small):
    """block payload sizes that put the seams where a reader can go wrong"""
    recs, stream, first = small
    b = _boundaries(stream, first)
    mid = b[5]
    one_per_block = [first] + [b[i + 1] - b[i] for i in range(len(b) - 1)]
    return {"block_size word split over two blocks": [mid + 2, 60000],
            "record body split over blocks": [mid + 4 + 17, 60000],
            "one record per block": one_per_block,
            "an empty data block": [first + 11, 0, 40, 0, 60000],
            "header split, 7-byte blocks": 7,
            "one block": 60000}


@pytest.mark.parametrize("case", ["block_size word split over two blocks", "record body split over blocks", "one record per block",
                                  "an empty data block", "header split, 7-byte blocks", "one block"])
def test_writer_to_reader_round_trip(tmp_path, small, case):
    from exomedepth_amd import bam
    recs, stream, first = small
    path = str(tmp_path / "t.bam")
    rck.write_bgzf(path, stream, _payloads(small)[case])
    slow = rck.parse_bam(path)
    _same(slow["records"], _expected(recs))
    with bam.BamFile(path) as b:
        assert b.ref_names == slow["ref_names"] == [r[0] for r in REFS]
        assert b.ref_lengths == slow["ref_lengths"] == [r[1] for r in REFS]
        assert b.text == slow["text"] == TEXT
        _same(b.records(), slow["records"])


@pytest.mark.parametrize("chunk", [1, 33, 4096, None])
def test_scanner_in_chunks(small, chunk):
    from exomedepth_amd import bam
    recs, stream, first = small
    body = stream[first:]
    bounds = {b - first for b in _boundaries(stream, first)}
    step = len(body) if chunk is None else chunk
    got, tail, at = [], b"", 0
    for p in range(0, len(body), step):
        buf = tail + body[p:p + step]
        rec, used = bam.scan_records(buf)
        at += used
        assert at in bounds                       # bytes_consumed always lands on a record boundary
        tail = buf[used:]
        got.append(rec)
    assert tail == b"" and at == len(body)
    _same(tuple(np.concatenate([g[k] for g in got]) for k in range(4)), _expected(recs))
    _same(tuple(np.concatenate([g[k] for g in bam.scan_stream(body[p:p + step] for p in range(0, len(body), step))]) for k in range(4)),
          _expected(recs))


def test_scanner_respects_cap(small):
    from exomedepth_amd import bam
    recs, stream, first = small
    b = _boundaries(stream, first)
    rec, used = bam.scan_records(stream[first:], cap=10)
    assert rec[0].size == 10 and used == b[10] - first
    rec, used = bam.scan_records(b"")
    assert rec[0].size == 0 and used == 0


def test_truncation_inside_the_last_record(small):
    from exomedepth_amd import bam
    recs, stream, first = small
    b = _boundaries(stream, first)
    body, last = stream[first:], b[-2] - first
    want = tuple(a[:-1] for a in _expected(recs))
    for cut in range(last, len(body)):
        rec, used = bam.scan_records(body[:cut])
        assert used == last
        _same(rec, want)
    with pytest.raises(ValueError, match="truncated BAM"):
        list(bam.scan_stream([body[:len(body) - 1]]))


@pytest.mark.parametrize("block_size", [31, 0, -1, 2**30, -2**31])
def test_bad_block_size_is_an_error(small, block_size):
    from exomedepth_amd import EdError, bam
    recs, stream, first = small
    b = _boundaries(stream, first)
    body = bytearray(stream[first:])
    at = b[3] - first
    body[at:at + 4] = struct.pack("<i", block_size)
    with pytest.raises(EdError, match=r"block_size %d .*status -1" % block_size):
        bam.scan_records(bytes(body))


def test_scanner_arguments():
    from exomedepth_amd import _lib
    n, used = C.c_int64(0), C.c_int64(0)
    assert _lib.lib().ed_bam_scan_records(None, -1, 0, None, None, None, None, C.byref(n), C.byref(used)) == -1
    assert _lib.lib().ed_bam_scan_records(None, 0, 0, None, None, None, None, None, C.byref(used)) == -1
    assert _lib.lib().ed_bam_scan_records(None, 0, 0, None, None, None, None, C.byref(n), C.byref(used)) == 0


def test_not_a_bam_file(tmp_path, small):
    from exomedepth_amd import bam
    recs, stream, first = small
    p = str(tmp_path / "x.bam")
    rck.write_bgzf(p, b"BAM\2" + stream[4:], 60000)                     # BGZF, wrong magic
    with pytest.raises(ValueError, match="not a BAM file"):
        bam.BamFile(p)
    open(p, "wb").write(b"@HD\tVN:1.0\n" * 20)                           # not BGZF at all
    with pytest.raises(ValueError, match="not a BGZF file"):
        bam.BamFile(p)
    open(p, "wb").write(b"")
    with pytest.raises(ValueError, match="not a BGZF file"):
        bam.BamFile(p)
    rck.write_bgzf(p, stream, 60000)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:len(raw) - 40])                            # cut inside the data block
    with pytest.raises(ValueError, match="truncated BGZF"):
        bam.BamFile(p).records()
    bad = bytearray(raw)
    bad[len(raw) - 28 - 8] ^= 0x55                                      # the data block's CRC-32
    open(p, "wb").write(bytes(bad))
    with pytest.raises(ValueError, match="corrupt BGZF block"):
        bam.BamFile(p).records()


def test_thread_count_comes_from_the_environment(monkeypatch):
    from exomedepth_amd import bam
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert bam.n_threads() == 3
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= bam.n_threads() <= 16


def test_fixture_figures():
    """what a throwaway parser read from the reference's example file; both parsers must find the same"""
    from exomedepth_amd import bam
    slow = rck.parse_bam(FIXTURE)
    assert (slow["n_blocks"], slow["n_inflated"], len(slow["ref_names"]), slow["records"][0].size) == (15, 821947, 86, 2208)
    assert np.all(slow["records"][0] == 0)
    with bam.BamFile(FIXTURE) as b:
        assert b.ref_names == slow["ref_names"] and b.ref_lengths == slow["ref_lengths"] and b.text == slow["text"]
        _same(b.records(), slow["records"])
    flag = slow["records"][3] & 0xFFFF
    keep = rck.fragments_getbamcounts(slow["records"], 20, 300)[0]
    assert int((keep & ((flag & 1) != 0)).sum()) == 464 and int((keep & ((flag & 1) == 0)).sum()) == 3
    assert int(rck.fragments_everted(slow["records"], 0)[0].sum()) == 7
    assert int(rck.fragments_everted(slow["records"], 35)[0].sum()) == 1


def _shuffled_frame():
    chrom = ["X", "10", "2", "MT", "2", "10", "X", "2", "10", "2", "MT", "X"]
    start = [500, 100, 300, 10, 100, 100, 50, 200, 90, 150, 5, 500]
    end = [600, 200, 400, 90, 200, 220, 80, 300, 210, 250, 95, 600]          # 10: (100,200) and (90,210) share start + end; so do X's two (500,600)
    name = ["e%d" % i for i in range(len(chrom))]
    return {"chromosome": chrom, "start": start, "end": end, "name": name}


@pytest.mark.parametrize("include_chr", [False, True])
def test_frame_preparation_row_and_column_order(include_chr, tmp_path):
    import exomedepth_amd as ed
    f = _shuffled_frame()
    t = ed.bed_targets(bed_frame=f, include_chr=include_chr)
    assert list(t.keys()) == ["chromosome", "start", "end", "exon"]
    # levels: 1..22 first (of those present: 2, 10), then first seen (X, MT); within a level by start + end, ties in input order
    want = [4, 9, 7, 2, 1, 8, 5, 6, 0, 11, 3, 10]
    pre = "chr" if include_chr else ""
    if include_chr:          # with the prefix no name is one of '1'..'22' any more: all levels in first-seen order (chrX, chr10, chr2, chrMT)
        want = [6, 0, 11, 1, 8, 5, 4, 9, 7, 2, 3, 10]
    assert list(t["chromosome"]) == [pre + f["chromosome"][i] for i in want]
    assert list(t["start"]) == [f["start"][i] + 1 for i in want] and t["start"].dtype == np.int32
    assert list(t["end"]) == [f["end"][i] for i in want]
    assert list(t["exon"]) == [f["name"][i] for i in want]
    k = ed.bed_targets(bed_frame=f, include_chr=include_chr, reorder=False)       # count.everted.reads keeps the caller's rows
    assert list(k["chromosome"]) == [pre + c for c in f["chromosome"]] and list(k["start"]) == [s + 1 for s in f["start"]]
    assert list(k["exon"]) == f["name"]
    three = ed.bed_targets(bed_frame=[f["chromosome"], f["start"], f["end"]])
    assert list(three.keys()) == ["chromosome", "start", "end"]
    numeric4 = ed.bed_targets(bed_frame=[f["chromosome"], f["start"], f["end"], list(range(12))])
    assert "exon" not in numeric4
    p = str(tmp_path / "t.bed")
    with open(p, "w") as fh:
        for i in range(12):
            fh.write("%s\t%d\t%d\t%s\n" % (f["chromosome"][i], f["start"][i], f["end"][i], f["name"][i]))
    u = ed.bed_targets(bed_file=p, include_chr=include_chr)
    assert all(list(u[c]) == list(t[c]) for c in t) and list(u.keys()) == list(t.keys())
    with pytest.raises(ValueError, match="bed"):
        ed.bed_targets()


def test_target_chromosome_missing_from_the_header():
    import exomedepth_amd as ed
    frame = {"chromosome": ["1", "nope", "chrZ"], "start": [25630000, 5, 7], "end": [25630200, 50, 70]}
    with pytest.raises(ValueError, match="nope, chrZ"):
        ed.getBamCounts(bed_frame=frame, bam_files=[FIXTURE])
    with pytest.raises(ValueError, match="chr1"):
        ed.count_everted_reads(bed_frame=frame, bam_files=FIXTURE, include_chr=True)
    with pytest.raises(ValueError, match="1 <= start <= end"):
        ed.getBamCounts(bed_frame={"chromosome": ["1"], "start": [50], "end": [50]}, bam_files=[FIXTURE])


def test_no_device_no_counter():
    import exomedepth_amd as ed
    from exomedepth_amd import EdError, _lib
    if _lib.lib().ed_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(EdError, match="no usable HIP device"):
        ed.ReadCounter(["1", "1"], [10, 30], [20, 40], 1)
    frame = {"chromosome": ["1"], "start": [25630000], "end": [25630200]}
    with pytest.raises(EdError, match="no usable HIP device"):
        ed.getBamCounts(bed_frame=frame, bam_files=[FIXTURE])
    with pytest.raises(EdError, match="no usable HIP device"):
        ed.count_everted_reads(bed_frame=frame, bam_files=[FIXTURE])
    with pytest.raises(EdError, match="1 <= start <= end"):             # validation comes before the device
        ed.ReadCounter(["1"], [0], [20], 1)
    g = ed.readcount_geometry()
    assert g["records_per_workgroup"] % g["block"] == 0 and g["block"] % 64 == 0
