"""Not a test: the slow, independent side of the read-count tests.

  * ref_getbamcounts / ref_everted: the two R functions (reference R/countBamInGranges.R) restated with numpy as an exon x fragment compare,
    the filters written out from the R lines.  Nothing here ranks, sorts or scans: it is the definition, not the method under test.
  * parse_bam: a BAM parser of its own -- gzip members inflated one after the other, one struct.unpack_from per record.
  * write_bam: a minimal BAM / BGZF writer, for files whose records straddle the blocks as a test wants them.
"""
import struct
import zlib

import numpy as np

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# --------------------------------------------------------------------------------------------- the two R functions
def _fields(records):
    refid, pos, tlen, fm = (np.asarray(a).astype(np.int64) for a in records)
    return refid, pos, tlen, fm & 0xFFFF, (fm >> 16) & 0xFF


def fragments_getbamcounts(records, min_mapq=20, read_width=300):
    """(keep, start, end) per record by countBamInGRanges.exomeDepth"""
    refid, pos, tlen, flag, mapq = _fields(records)
    bit = lambda b: (flag & b) != 0
    ok_mapq = (mapq != 255) & (mapq > min_mapq)                               # :224, :238 `mapq > min.mapq`; 255 is NA in R (stated deviation)
    # :218-219 isDuplicate = F, isUnmappedQuery = F, hasUnmappedMate = F, isPaired = T, isProperPair = T, isSecondaryAlignment = F; :224 isize > 0
    paired = bit(0x1) & bit(0x2) & ~bit(0x4) & ~bit(0x8) & ~bit(0x100) & ~bit(0x400) & ok_mapq & (tlen > 0)
    # :232 isDuplicate = F, isPaired = F, isSecondaryAlignment = F; an unmapped read has no alignment for readGAlignments
    single = ~bit(0x1) & ~bit(0x4) & ~bit(0x100) & ~bit(0x400) & ok_mapq
    start = pos + 1
    end = np.where(paired, start + tlen, start + read_width)                  # :227 start + isize; :241 start + read.width
    return paired | single, start, end


def fragments_everted(records, min_mapq=20):
    """(keep, start, end) per record by countBam.everted"""
    refid, pos, tlen, flag, mapq = _fields(records)
    bit = lambda b: (flag & b) != 0
    # :127 isDuplicate = F, isPaired = T, isProperPair = F, isSecondaryAlignment = F; unmapped reads left out (stated deviation)
    flags_ok = bit(0x1) & ~bit(0x2) & ~bit(0x100) & ~bit(0x400) & ~bit(0x4)
    forward = ~bit(0x10)
    # :130
    keep = flags_ok & (mapq != 255) & (mapq >= min_mapq) & (pos >= 0) & (np.abs(tlen) < 100000) & ((forward & (tlen < 0)) | (~forward & (tlen > 0)))
    p1 = pos + 1
    return keep, np.minimum(p1, p1 + tlen), np.maximum(p1, p1 + tlen)         # :136 pmin / pmax


def count_overlaps(exon_chrom, exon_start, exon_end, frag_chrom, frag_start, frag_end):
    """countOverlaps(exons, fragments), type any, closed ranges: exon x fragment compare (in slabs of exons)"""
    exon_chrom, exon_start, exon_end = (np.asarray(a).astype(np.int64) for a in (exon_chrom, exon_start, exon_end))
    out = np.zeros(exon_start.size, np.int64)
    step = max(1, 20_000_000 // max(1, frag_start.size))
    for e0 in range(0, exon_start.size, step):
        s = slice(e0, e0 + step)
        hit = ((frag_chrom[None, :] == exon_chrom[s, None]) & (frag_start[None, :] <= exon_end[s, None])
               & (frag_end[None, :] >= exon_start[s, None]))
        out[s] = hit.sum(axis=1)
    return out


def ref_counts(mode, exon_chrom, exon_start, exon_end, records, ref_to_chrom, min_mapq=20, read_width=300):
    """what ReadCounter.add + finish must give for these records: int64 per exon.  exon_chrom: ids; ref_to_chrom[refid] -> id or -1"""
    refid = np.asarray(records[0]).astype(np.int64)
    r2c = np.asarray(ref_to_chrom).astype(np.int64)
    inside = (refid >= 0) & (refid < r2c.size)
    chrom = np.where(inside, r2c[np.clip(refid, 0, max(r2c.size - 1, 0))] if r2c.size else -1, -1)
    keep, fs, fe = fragments_getbamcounts(records, min_mapq, read_width) if mode == 0 else fragments_everted(records, min_mapq)
    keep = keep & (chrom >= 0)
    return count_overlaps(exon_chrom, exon_start, exon_end, chrom[keep], fs[keep], fe[keep])


# --------------------------------------------------------------------------------------------- a BAM parser of its own
def parse_bam(path):
    """dict(n_blocks, n_inflated, text, ref_names, ref_lengths, records = (refid, pos, tlen, flag_mapq)); slow on purpose"""
    raw = open(path, "rb").read()
    data, n_blocks, off = bytearray(), 0, 0
    while off < len(raw):
        d = zlib.decompressobj(31)                        # one gzip member
        data += d.decompress(raw[off:])
        assert d.eof, "truncated gzip member"
        off = len(raw) - len(d.unused_data)
        n_blocks += 1
    data = bytes(data)
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text]
    n_ref, = struct.unpack_from("<i", data, 8 + l_text)
    p = 12 + l_text
    names, lengths = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, p)
        names.append(data[p + 4:p + 4 + l_name - 1].decode())
        lengths.append(struct.unpack_from("<i", data, p + 4 + l_name)[0])
        p += 8 + l_name
    rows = []
    while p < len(data):
        block_size, refid, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, next_refid, next_pos, tlen = struct.unpack_from("<iiiBBHHHIiii", data, p)
        rows.append((refid, pos, tlen, flag | (mapq << 16)))
        p += 4 + block_size
    assert p == len(data)
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return {"n_blocks": n_blocks, "n_inflated": len(data), "text": text.split(b"\0")[0].decode(), "ref_names": names, "ref_lengths": lengths,
            "records": (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.uint32))}


# --------------------------------------------------------------------------------------------- a minimal writer
def bam_stream(text, refs, records):
    """the inflated stream and the offset where the records begin.  refs: [(name, length)]; records: tuples
    (refid, pos, mapq, flag, tlen[, name_len[, n_cigar[, l_seq]]]) -- a read name, CIGAR and bases of the chosen lengths are made up"""
    t = text.encode()
    out = bytearray(b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs)))
    for name, length in refs:
        nm = name.encode() + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", length)
    first = len(out)
    for k, r in enumerate(records):
        refid, pos, mapq, flag, tlen = r[:5]
        name_len = r[5] if len(r) > 5 else 1 + k % 7
        n_cigar = r[6] if len(r) > 6 else k % 3
        l_seq = r[7] if len(r) > 7 else k % 5
        name = (b"r%d" % k).ljust(name_len, b"x")[:name_len] + b"\0"
        body = struct.pack("<iiBBHHHIiii", refid, pos, len(name), mapq, 4680, n_cigar, flag, l_seq, -1, -1, tlen)
        body += name + struct.pack("<%dI" % n_cigar, *[(10 << 4) | 0] * n_cigar) + bytes((l_seq + 1) // 2) + bytes([30]) * l_seq
        out += struct.pack("<i", len(body)) + body
    return bytes(out), first


def bgzf_block(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(payload) + c.flush()
    size = 18 + len(comp) + 8
    assert size <= 65536
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, size - 1) + comp
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def write_bgzf(path, stream, payload_sizes, eof=True):
    """the stream cut into BGZF blocks: payload_sizes is a number (every block that long) or a list of lengths (0 = an empty data block),
    cycled until the stream is used up"""
    sizes = [payload_sizes] if np.isscalar(payload_sizes) else list(payload_sizes)
    assert max(sizes) > 0
    with open(path, "wb") as f:
        p = k = 0
        while p < len(stream):
            n = sizes[k % len(sizes)]
            f.write(bgzf_block(stream[p:p + n]))
            p += n
            k += 1
        if eof:
            f.write(EOF_BLOCK)


def write_bam(path, text, refs, records, payload_sizes=60000):
    stream, first = bam_stream(text, refs, records)
    write_bgzf(path, stream, payload_sizes)
    return stream, first
