"""BAM files on the device (csrc/edinflate.inc through ed_bamdev_*, ed_readcount_add_device; bam.DeviceInflater, bam.DeviceBamFile,
ReadCounter.add_device, getBamCounts(inflate="device")).  The inflater against Python's zlib on the blocks of tests/inflate_cases.py -- the ones
the host checker (tests/test_inflate_host.py) runs; the record scan against the host route (bam.BamFile, ed_bam_scan_records).  Bytes, integers
and statuses: every comparison is exact equality."""
import os
import struct

import pytest

import inflate_cases as ic
import readcount_checker as rck

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "minimum_1_25630000_25650000.bam")
GAP = 64
GUARD = 0xA5


@pytest.fixture(scope="module")
def bam():
    import exomedepth_amd                                   # noqa: F401  (loads the library)
    from exomedepth_amd import bam as _bam
    return _bam


@pytest.fixture(scope="module")
def good():
    return ic.cases()


def _run(bam, blocks, gap=GAP, batch_bytes=64 << 20):
    """the blocks as one file through a DeviceInflater: (error or None, statuses, the raw output with its guard bytes) of the last batch"""
    data = b"".join(blocks)
    with bam.DeviceInflater(0, batch_bytes) as d:
        d.begin(gap=gap)
        err, off = None, 0
        try:
            while off < len(data):
                used = d.push(data[off:])
                assert used > 0
                off += used
            d.end()
        except Exception as e:                               # the statuses and bytes of the batch that failed are still there
            err = e
        return err, d.statuses(), d.inflated()


def _slots(raw, payload_sizes, gap=GAP):
    """the blocks' bytes out of the raw output; every guard byte before, between and after the slots must be untouched"""
    out, p = [], 0
    for n in payload_sizes:
        assert (raw[p:p + gap] == GUARD).all()
        out.append(raw[p + gap:p + gap + n].tobytes())
        p += gap + n
    assert (raw[p:p + gap] == GUARD).all() and p + gap == raw.size
    return out


def test_geometry(bam):
    g = bam.bamdev_geometry()
    assert g["scan_blocks_per_workgroup"] >= 64
    assert g["threads"] == 64 * g["blocks_per_workgroup"] and 0 < g["lds_bytes_per_block"] * g["blocks_per_workgroup"] <= 64 << 10


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_inflate_parity(bam, good, order):
    cases = good if order == "forward" else good[::-1]
    err, status, raw = _run(bam, [b for _, b, _ in cases])
    assert err is None
    assert status.size == len(cases) and (status == 0).all(), [(cases[k][0], bam.INFLATE_STATUS[s]) for k, s in enumerate(status) if s]
    got = _slots(raw, [len(p) for _, _, p in cases])
    for (name, _, p), g in zip(cases, got):
        assert g == p, name


def test_inflate_without_gap_is_one_stream(bam, good):
    err, status, raw = _run(bam, [b for _, b, _ in good], gap=0)
    assert err is None and raw.tobytes() == b"".join(p for _, _, p in good)


def test_refusals(bam, good):
    """bad blocks among good ones: each bad one gets its status, each good one its bytes, nothing outside a block's slot is touched, and the
    call that waits for the batch names the first bad block"""
    bad = ic.bad_blocks()
    dyn = [b for n, b, _ in ic.small_blocks() if n == "dynamic"][0]
    corrupt = ic.corruptions(dyn)                           # every labelled single-byte corruption (the host checker ran them first)
    some = [c for c in good if len(c[1]) < 4000][:12]
    rows = []                                               # (name, block, payload or None, status name or None)
    for k, (name, b, st) in enumerate(bad):
        rows.append(some[k % len(some)] + (None,))
        rows.append((name, b, None, st))
    for k, (c, p) in enumerate(corrupt):
        rows.append(("corruption %d" % k, c, p, None))
    rows.append(some[0] + (None,))
    sizes = [struct.unpack_from("<I", b, len(b) - 4)[0] for _, b, _, _ in rows]
    def whole(b):                                           # a corrupted gzip header or BSIZE never reaches the decoder: the file is cut by them
        try:
            return bam._block_size(b, 0) == len(b)
        except ValueError:
            return False
    # (a corrupted ISIZE above 64 KiB is refused before any device work: next test)
    keep = [k for k, n in enumerate(sizes) if n <= 65536 and whole(rows[k][1])]
    rows, sizes = [rows[k] for k in keep], [sizes[k] for k in keep]
    err, status, raw = _run(bam, [r[1] for r in rows])
    got = _slots(raw, sizes)
    first_bad = None
    for k, (name, b, p, st) in enumerate(rows):
        if p is not None:
            assert status[k] == 0 and got[k] == p, name
        else:
            assert status[k] != 0, name
            if st is not None:
                assert bam.INFLATE_STATUS[status[k]] == st, (name, bam.INFLATE_STATUS[status[k]])
            if first_bad is None:
                first_bad = k
    assert any(bam.INFLATE_STATUS[s] == "INPUT_OVERRUN" for s in status)
    at = sum(len(r[1]) for r in rows[:first_bad])
    assert err is not None and "block %d of the file, at byte %d," % (first_bad, at) in str(err)
    assert bam.INFLATE_STATUS[status[first_bad]] in str(err)


def test_refused_before_device_work(bam, good):
    b = good[5][1]
    with bam.DeviceInflater(0, 1 << 20) as d:
        d.begin()
        with pytest.raises(Exception, match="inflated size of 65537"):
            d.push(b[:-4] + struct.pack("<I", 65537))
        d.begin()
        with pytest.raises(Exception, match="no BGZF block header at byte 0"):
            d.push(b"\x1f\x8b\x08\x00" + b[4:])
        d.begin()
        assert d.push(b[:-1]) == 0 and d.push(b[:11]) == 0 and d.push(b"") == 0      # an incomplete block is left to the caller
        d.end()


def test_geometry_edges_and_batches(bam, good):
    """block counts one fewer than, exactly and one more than a workgroup's worth; and the same file cut into batches that end at every block"""
    w = bam.bamdev_geometry()["blocks_per_workgroup"]
    small = [c for c in good if len(c[1]) < 2000]
    for n in (w - 1, w, w + 1, 2 * w + 1):
        cases = [small[k % len(small)] for k in range(n)]
        err, status, raw = _run(bam, [b for _, b, _ in cases])
        assert err is None and (status == 0).all() and _slots(raw, [len(p) for _, _, p in cases]) == [p for _, _, p in cases]
    cases = small[:9]
    data = b"".join(b for _, b, _ in cases)
    want = b"".join(p for _, _, p in cases)
    with bam.DeviceInflater(0, 1) as d:                       # batch_bytes = 1: a block a batch, two in flight
        d.begin()
        got, off, pending = b"", 0, False
        while off < len(data):
            used = d.push(data[off:])
            if pending:
                got += d.inflated().tobytes()
            pending = True
            off += used
        d.end()
        got += d.inflated().tobytes()
        assert got == want and d.kernel_ms()[0] > 0.0


@pytest.mark.parametrize("batch_bytes", [32 << 20, 3000])
def test_inflated_device_route(bam, tmp_path, batch_bytes):
    """bam.inflated(device=0) gives the host route's stream, byte for byte, for the bundled file and for written ones"""
    recs = [(k % 2, 100 + 7 * k, 30, 0x3, 40 + k % 50) for k in range(3000)]
    paths = [FIXTURE]
    for size in (60000, 4096, 37):
        paths.append(str(tmp_path / ("w%d.bam" % size)))
        rck.write_bam(paths[-1], "@HD\tVN:1.0\n", [("1", 10 ** 6), ("2", 10 ** 6)], recs, payload_sizes=size)
    for path in paths:
        host = b"".join(bam.inflated(path, batch_bytes=batch_bytes))
        dev = b"".join(bam.inflated(path, batch_bytes=batch_bytes, device=0))
        assert dev == host, path


def test_inflated_device_errors(bam, tmp_path, good):
    """the same errors for the same files"""
    p = str(tmp_path / "bad.bam")
    blocks = [good[9][1], good[13][1], good[17][1]]
    broken = blocks[1][:-8] + bytes([blocks[1][-8] ^ 0x10]) + blocks[1][-7:]
    open(p, "wb").write(blocks[0] + broken + blocks[2])
    with pytest.raises(ValueError, match="corrupt BGZF block"):
        list(bam.inflated(p))
    with pytest.raises(ValueError, match="corrupt BGZF block: block 1 of the file, at byte %d, does not inflate: BAD_CRC" % len(blocks[0])):
        list(bam.inflated(p, device=0))
    open(p, "wb").write(blocks[0] + blocks[2][:-5])
    for dev in (None, 0):
        with pytest.raises(ValueError, match="truncated BGZF file: %d bytes after the last whole block" % (len(blocks[2]) - 5)):
            list(bam.inflated(p, device=dev))
    open(p, "wb").write(b"")
    for dev in (None, 0):
        with pytest.raises(ValueError, match="not a BGZF file: it is empty"):
            list(bam.inflated(p, device=dev))


def test_counts_by_both_routes(bam, tmp_path):
    """getBamCounts and count_everted_reads give the same frame with the blocks inflated on the device as on the host: the bundled file, and a
    two-file cohort of written files whose records straddle the blocks"""
    import numpy as np
    import exomedepth_amd as ed
    s = np.arange(25630000, 25650000, 500)
    tiles = {"chromosome": ["1"] * s.size, "start": s, "end": s + 500}
    spans = {"chromosome": ["1", "1"], "start": [2580000, 2610000], "end": [2610000, 2640000]}
    recs = [(k % 2, 1000 + 11 * k, 30 + k % 3, (0x1 | 0x2) if k % 3 else (0x1 | 0x10), 200 - 90 * (k % 3 == 0)) for k in range(4000)]
    written = []
    for size in (4096, 37):
        written.append(str(tmp_path / ("c%d.bam" % size)))
        rck.write_bam(written[-1], "@HD\tVN:1.0\n", [("1", 10 ** 6), ("2", 10 ** 6)], recs, payload_sizes=size)
    grid = {"chromosome": ["1"] * 50 + ["2"] * 50, "start": list(range(0, 50000, 1000)) * 2, "end": list(range(1000, 51000, 1000)) * 2}
    for frame, files in ((tiles, [FIXTURE]), (grid, written)):
        host = ed.getBamCounts(bed_frame=frame, bam_files=files)
        dev = ed.getBamCounts(bed_frame=frame, bam_files=files, inflate="device")
        assert list(host.keys()) == list(dev.keys())
        for k in host:
            assert np.array_equal(np.asarray(host[k]), np.asarray(dev[k])), k
        assert sum(int(np.asarray(host[os.path.basename(f)]).sum()) for f in files) > 0
    for frame, files in ((spans, [FIXTURE]), (grid, written)):
        host = ed.count_everted_reads(bed_frame=frame, bam_files=files, min_mapq=0)
        dev = ed.count_everted_reads(bed_frame=frame, bam_files=files, min_mapq=0, inflate="device")
        for k in host:
            assert np.array_equal(np.asarray(host[k]), np.asarray(dev[k])), k
    with pytest.raises(ValueError, match="inflate must be"):
        ed.getBamCounts(bed_frame=tiles, bam_files=[FIXTURE], inflate="gpu")


# ------------------------------------------------------------------------------------------------ the record scan on the device
REFS = [("1", 10 ** 6), ("2", 10 ** 6)]


def _recs(n):
    return [(k % 2, 100 + 7 * k, k % 61, 0x3 if k % 3 else 0x11, 150 - (k % 5) * 60) for k in range(n)]


def _same(a, b):
    import numpy as np
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """files from the tests' writer: payloads of 60 000, 4 096, 37 (a record's fixed part straddles a boundary) and 1 byte a block"""
    d = tmp_path_factory.mktemp("bamdev")
    out = {}
    for size, n in ((60000, 3000), (4096, 3000), (37, 600), (1, 40)):
        out[size] = str(d / ("p%d.bam" % size))
        rck.write_bam(out[size], "@HD\tVN:1.0\n", REFS, _recs(n), payload_sizes=size)
    return out


@pytest.mark.parametrize("which", ["fixture", 60000, 4096, 37, 1])
def test_scan_parity(bam, written, which):
    """the four arrays equal BamFile(path).records(), in one batch and in batches that end inside records"""
    path = FIXTURE if which == "fixture" else written[which]
    want = bam.BamFile(path).records()
    assert want[0].size > 0
    for batch_bytes in (32 << 20, 5000, 700, 1):             # 1: a block a batch -- batches end in block_size words, fixed parts and tails
        f = bam.DeviceBamFile(path, batch_bytes=batch_bytes)
        assert _same(f.records(), want), (which, batch_bytes)
    assert f.ref_names == bam.BamFile(path).ref_names and sum(f.kernel_ms) > 0.0


def test_scan_batches_end_inside_a_record(bam, tmp_path):
    """blocks cut so that a batch (a block) ends inside a block_size word, inside a fixed part and inside a tail"""
    stream, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, _recs(50))
    bs = struct.unpack_from("<i", stream, first)[0]
    second = first + 4 + bs
    cuts = [first + 2, second + 4 + 10, second + 4 + 32 + 3]     # in the word of record 0, in the fixed part of record 1, in its tail
    sizes = [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], len(stream) - cuts[2]]
    path = str(tmp_path / "cuts.bam")
    rck.write_bgzf(path, stream, sizes)
    want = bam.BamFile(path).records()
    assert want[0].size == 50
    for batch_bytes in (1, 32 << 20):
        assert _same(bam.DeviceBamFile(path, batch_bytes=batch_bytes).records(), want)


def test_scan_edge_files(bam, tmp_path):
    import numpy as np
    p = str(tmp_path / "e.bam")
    rck.write_bam(p, "@HD\tVN:1.0\n", REFS, [])             # no records
    assert all(a.size == 0 for a in bam.DeviceBamFile(p).records())
    text = "@HD\tVN:1.0\n" + "".join("@CO\t%s\n" % ("x" * 70) for _ in range(3000))
    recs = _recs(200)
    rck.write_bam(p, text, REFS, recs, payload_sizes=60000)   # a header that fills more than one block
    f = bam.DeviceBamFile(p)
    assert f.first_record_offset > 3 * 60000
    want = bam.BamFile(p).records()
    for batch_bytes in (32 << 20, 1):
        assert _same(bam.DeviceBamFile(p, batch_bytes=batch_bytes).records(), want)
    stream, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, recs)
    for cut in (1, 5, 40):                                   # a file whose last record is cut
        rck.write_bgzf(p, stream[:-cut], 4096)
        for make in (lambda: bam.BamFile(p).records(), lambda: bam.DeviceBamFile(p).records(), lambda: bam.DeviceBamFile(p, batch_bytes=1).records()):
            with pytest.raises(ValueError, match="truncated BAM: %d bytes of an incomplete record" % (len(stream) - cut - _last(stream, first))):
                make()
    for value in (31, -1, (1 << 28) + 1):                     # a bad block_size word planted mid-file
        offs = _offsets(stream, first)
        at = offs[120]
        broken = stream[:at] + struct.pack("<i", value) + stream[at + 4:]
        rck.write_bgzf(p, broken, 4096)
        host_rec, _ = None, None
        with pytest.raises(Exception) as host:
            bam.scan_records(broken[first:])
        msg = "record 120 at byte %d has block_size %d" % (at - first, value)
        assert msg in str(host.value)
        for batch_bytes in (32 << 20, 1):
            got = []
            with pytest.raises(Exception) as dev:
                for r in bam.DeviceBamFile(p, batch_bytes=batch_bytes).batches():
                    got.append(r.to_host())
            assert msg in str(dev.value), str(dev.value)
            got = tuple(np.concatenate([g[k] for g in got]) for k in range(4))
            assert _same(got, tuple(a[:120] for a in bam.BamFile(_good(tmp_path, stream)).records()))


def _offsets(stream, first):
    out, p = [], first
    while p < len(stream):
        out.append(p)
        p += 4 + struct.unpack_from("<i", stream, p)[0]
    return out


def _last(stream, first):
    return _offsets(stream, first)[-1]


def _good(tmp_path, stream):
    p = str(tmp_path / "good.bam")
    rck.write_bgzf(p, stream, 4096)
    return p


def test_scan_geometry_edges(bam, tmp_path):
    """block counts one fewer than, exactly and one more than a scan workgroup's worth, aligned and straddling"""
    w = bam.bamdev_geometry()["scan_blocks_per_workgroup"]
    stream, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, _recs(2 * w + 40))
    offs = _offsets(stream, first) + [len(stream)]
    p = str(tmp_path / "g.bam")
    for n in (w - 1, w, w + 1):
        # n data blocks that start on record boundaries: the header, then n - 1 blocks of one record or more
        sizes = [first] + [offs[k + 1] - offs[k] for k in range(n - 2)] + [len(stream) - offs[n - 2]]
        rck.write_bgzf(p, stream, sizes, eof=False)
        assert rck.parse_bam(p)["n_blocks"] == n
        assert _same(bam.DeviceBamFile(p).records(), bam.BamFile(p).records())
        size = -(-len(stream) // n)                           # and n blocks of one size: records straddle every block
        rck.write_bgzf(p, stream, size, eof=False)
        assert _same(bam.DeviceBamFile(p).records(), bam.BamFile(p).records())


def test_add_device_equals_host_fed_matrix(bam, written):
    import numpy as np
    import exomedepth_amd as ed
    chrom, start = ["1"] * 40 + ["2"] * 40, list(range(1, 40001, 1000)) * 2
    end = [s + 999 for s in start]
    for mode in (0, 1):
        rc = ed.ReadCounter(chrom, start, end, 2)
        try:
            f = bam.DeviceBamFile(written[4096], batch_bytes=9000)
            for rec in f.batches():
                rc.add_device(0, rec, f.ref_names, mode=mode, min_mapq=10)
            rc.finish(0)
            with bam.BamFile(written[4096]) as b:
                for rec in b.chunks():
                    rc.add(1, rec, b.ref_names, mode=mode, min_mapq=10)
            rc.finish(1)
            m = rc.device_counts().to_host()
            assert m[0].sum() > 0 and np.array_equal(m[0], m[1])
            with pytest.raises(Exception, match="column 5 outside"):          # refused before anything is read
                rc.add_device(5, bam.DeviceRecords(None, 1, (8, 8, 8, 8)), f.ref_names)
        finally:
            rc.close()


# ------------------------------------------------------------------------------------------------ the 64-lane executor at its edges
@pytest.fixture(scope="module")
def lane():
    return ic.lane_cases()


@pytest.mark.parametrize("order", ["forward", "reversed", "on every wavefront"])
def test_lane_edges(bam, lane, order):
    """the hand-made blocks of inflate_cases.lane_cases (pending literals x distance x length, dependent chains, mixed block types, tables zlib
    never writes, ISIZE at the CRC slices' edges) against zlib's bytes, with guard bytes around every slot; in both orders, and each block four
    times in a row, so that it is decoded by each of the workgroup's wavefronts"""
    w = bam.bamdev_geometry()["blocks_per_workgroup"]
    cases = {"forward": list(lane), "reversed": list(lane)[::-1], "on every wavefront": [c for c in lane for _ in range(w)]}[order]
    assert len(ic.triples()) >= 1500 and w >= 4
    err, status, raw = _run(bam, [b for _, b, _ in cases])
    assert err is None
    assert status.size == len(cases) and (status == 0).all(), [(cases[k][0], bam.INFLATE_STATUS[s]) for k, s in enumerate(status) if s]
    got = _slots(raw, [len(p) for _, _, p in cases])
    for k, ((name, _, p), g) in enumerate(zip(cases, got)):
        assert g == p, (name, k)


def test_lane_refusals(bam, lane):
    """inflate_cases.lane_bad_blocks among good blocks: each bad one gets the status it is listed with, each neighbour its bytes, the guard bytes
    stand, and the call that waits for the batch names the first bad block"""
    bad = ic.lane_bad_blocks()
    some = [c for c in lane if len(c[1]) < 4000]
    rows = []                                               # (name, block, payload or None, status name)
    for k, (name, b, st) in enumerate(bad):
        rows.append(some[k % len(some)] + (None,))
        rows.append((name, b, None, st))
    rows.append(some[0] + (None,))
    sizes = [struct.unpack_from("<I", b, len(b) - 4)[0] for _, b, _, _ in rows]
    err, status, raw = _run(bam, [r[1] for r in rows])
    got = _slots(raw, sizes)
    assert status.size == len(rows)
    for k, (name, b, p, st) in enumerate(rows):
        if p is not None:
            assert status[k] == 0 and got[k] == p, name
        else:
            assert bam.INFLATE_STATUS[status[k]] == st, (name, bam.INFLATE_STATUS[status[k]])
    assert {st for _, _, st in bad} == {"BAD_SYMBOL", "BAD_CODE_LENGTHS", "BAD_DISTANCE", "OUTPUT_OVERRUN"}
    assert err is not None and "block 1 of the file, at byte %d," % len(rows[0][1]) in str(err) and bad[0][2] in str(err)


# ------------------------------------------------------------------------------------------------ the record scan where a wrong guess succeeds
DECOY = (777, 0x12345678, -77777, 0xBEEF | (0xAB << 16))     # refID, pos, tlen, flag | mapq << 16 of the fake records: nowhere else in the files


def _raw_record(refid, pos, mapq, flag, tlen, tail=b""):
    """a record of the 32 fixed bytes and `tail` (no read name, no CIGAR, no bases: to the scanner a record is its block_size word and its fixed part)"""
    body = struct.pack("<iiBBHHHIiii", refid, pos, 0, mapq, 4680, 0, flag, 0, -1, -1, tlen) + tail
    return struct.pack("<i", len(body)) + body


def _fake(tail_bytes=8):
    return _raw_record(DECOY[0], DECOY[1], DECOY[3] >> 16, DECOY[3] & 0xFFFF, DECOY[2], b"\x55" * tail_bytes)


def _decoy_file(path, variant):
    """a file with one record whose tail is a chain of fake records, and a BGZF block cut to begin at the first of them.  The walk from that
    block's first byte (the guess) goes along the fakes and then (a) arrives at the true record's end inside the block and goes on along true
    records, (b) meets a bad block_size word, (c) meets a block_size that reaches past the end of the file, (d) leaves the block exactly at the
    next block's first byte, which is the true record's end"""
    head, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, _recs(20))
    after, first2 = rck.bam_stream("@HD\tVN:1.0\n", REFS, _recs(60))
    after = after[_offsets(after, first2)[20]:]              # records 20 .. 59 of the same kind
    pad = b"\x01" * 10
    tail = pad + b"".join(_fake(8 * (k % 3)) for k in range(5))
    if variant == "b":
        tail += struct.pack("<i", 7) + b"\x02" * 40
    elif variant == "c":
        tail += struct.pack("<i", 1 << 27) + b"\x02" * 40
    rec = _raw_record(1, 5000, 33, 0x3, 150, tail)
    decoy_at = len(head) + 36 + len(pad)                     # the first fake's block_size word
    stream = head + rec + after
    true_end = len(head) + len(rec)
    if variant == "d":
        sizes = [decoy_at, true_end - decoy_at, 700, len(stream)]
    else:
        sizes = [decoy_at, true_end - decoy_at + 700 + 13, 500, len(stream)]     # the block goes on through true records and ends inside one
    rck.write_bgzf(path, stream, sizes)
    # what the guess walks over, by the scanner's own rule: the fakes parse as a chain that starts at the block's first byte
    got = struct.unpack_from("<iii", stream, decoy_at)
    assert got[0] >= 32 and got[1:] == DECOY[:2]
    return stream, first


@pytest.mark.parametrize("variant", ["a", "b", "c", "d"])
def test_scan_decoy_chain(bam, tmp_path, variant):
    import numpy as np
    p = str(tmp_path / "decoy.bam")
    _decoy_file(p, variant)
    want = bam.BamFile(p).records()
    assert want[0].size == 61 and not any((w == np.asarray(v).astype(w.dtype)).any() for w, v in zip(want, DECOY))
    for batch_bytes in (32 << 20, 1):
        got = bam.DeviceBamFile(p, batch_bytes=batch_bytes).records()
        assert _same(got, want), (variant, batch_bytes)
        assert not any((g == np.asarray(v).astype(g.dtype)).any() for g, v in zip(got, DECOY))


EMPTY_AT = (0, 1, 255, 256, 257)


@pytest.mark.parametrize("straddle", [False, True])
def test_scan_empty_blocks_mid_file(bam, tmp_path, straddle):
    """empty data blocks, as a concatenated BGZF file has them, as the first, second, 256th, 257th and 258th data block and as the last one before
    the end-of-file block; blocks cut at record boundaries, and at a fixed payload so that records straddle them"""
    n = 300
    stream, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, _recs(n))
    offs = _offsets(stream, first) + [len(stream)]
    data = [50] * (-(-(len(stream) - first) // 50)) if straddle else [offs[k + 1] - offs[k] for k in range(n)]
    for k in EMPTY_AT:
        data.insert(k, 0)
    assert len(data) > 258 and all(data[k] == 0 for k in EMPTY_AT) and sum(data) >= len(stream) - first
    p = str(tmp_path / "empty.bam")
    rck.write_bgzf(p, stream, [first] + data, eof=False)
    with open(p, "ab") as f:
        f.write(rck.bgzf_block(b"") + rck.EOF_BLOCK)
    assert rck.parse_bam(p)["n_blocks"] == 1 + len(data) + 2 <= 600
    want = bam.BamFile(p).records()
    assert want[0].size == n
    for batch_bytes in (32 << 20, 1):
        assert _same(bam.DeviceBamFile(p, batch_bytes=batch_bytes).records(), want), (straddle, batch_bytes)


@pytest.mark.parametrize("place", ["first", "middle", "last"])
def test_scan_record_longer_than_a_block(bam, tmp_path, place):
    """one record of 180 KB (l_seq = 120 000) among short ones: it spans four BGZF blocks of 60 000 bytes"""
    recs = _recs(30)
    at = {"first": 0, "middle": 15, "last": 30}[place]
    recs.insert(at, (1, 424242, 44, 0x3, 99, 5, 1, 120000))
    p = str(tmp_path / "long.bam")
    stream, first = rck.write_bam(p, "@HD\tVN:1.0\n", REFS, recs, payload_sizes=60000)
    offs = _offsets(stream, first) + [len(stream)]
    assert offs[at + 1] - offs[at] > 65536 and offs[at + 1] // 60000 - offs[at] // 60000 >= 3
    want = bam.BamFile(p).records()
    assert want[0].size == 31 and want[1][at] == 424242
    for batch_bytes in (32 << 20, 1):
        assert _same(bam.DeviceBamFile(p, batch_bytes=batch_bytes).records(), want), (place, batch_bytes)


def test_scan_densest_stream(bam, tmp_path):
    """records of block_size 32 -- 36 bytes each, the shortest the scanner takes -- in more than 256 blocks of 4 096 bytes: the record arrays' room
    (total / 36 + 1) is used to the last element but the header's share"""
    import numpy as np
    n = 30000
    head, first = rck.bam_stream("@HD\tVN:1.0\n", REFS, [])
    stream = head + b"".join(_raw_record(k % 2, 100 + 3 * k, k % 61, 0x3 if k % 3 else 0x11, 150 - (k % 5) * 60) for k in range(n))
    p = str(tmp_path / "dense.bam")
    rck.write_bgzf(p, stream, 4096)
    assert 256 < rck.parse_bam(p)["n_blocks"] <= 600 and len(stream) == first + 36 * n
    want = bam.BamFile(p).records()
    assert want[0].size == n and np.array_equal(want[1], 100 + 3 * np.arange(n, dtype=np.int32))
    for batch_bytes in (32 << 20, 1):
        assert _same(bam.DeviceBamFile(p, batch_bytes=batch_bytes).records(), want), batch_bytes
