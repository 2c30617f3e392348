"""Where the bases of a FASTA file lie, with the standard library and numpy only (no pysam, no samtools).

An uncompressed FASTA file is a series of records: a header line ('>' name, then an optional description) and the sequence in lines of one
length, the last possibly shorter.  Five numbers per record -- the `.fai` record of `samtools faidx` -- turn a base coordinate into a file
byte address without reading the file: the sequence's length, the byte offset of its first base, the bases per line and the bytes per line
(bases plus the line end).  FastaIndex reads them from `path + ".fai"` when that file exists, and otherwise builds them with one scan of the
file; byte_range() turns targets into byte ranges, which is all the device counter (ed_gc, csrc/edgc.inc) is given.
"""
import os

import numpy as np

_SCAN_BYTES = 1 << 26          # bytes of one step of the line-end scan


def _map(path, size):
    return np.memmap(path, dtype=np.uint8, mode="r") if size else np.zeros(0, np.uint8)


class FastaIndex:
    """One record per sequence of the FASTA file `path`: names (the header up to the first whitespace), and int64 arrays length, offset (file
    byte of the first base), line_bases and line_width (bytes of a line, its end included).  Read from path + ".fai" when that exists (and
    checked against the file: ValueError if stale), else built from the file itself (ValueError for what `samtools faidx` refuses)."""

    def __init__(self, path):
        self.path = os.fspath(path)
        self.size = os.path.getsize(self.path)
        with open(self.path, "rb") as f:
            if f.read(2) == b"\x1f\x8b":
                raise ValueError("%s is gzip-compressed (plain gzip or bgzip): compressed FASTA is not supported, decompress it first" % self.path)
        fai = self.path + ".fai"
        self.from_fai = os.path.exists(fai)
        rec = self._read_fai(fai) if self.from_fai else self._scan()
        self.names = [r[0] for r in rec]
        cols = np.asarray([r[1:] for r in rec], dtype=np.int64).reshape(len(rec), 4)
        self.length, self.offset, self.line_bases, self.line_width = (np.ascontiguousarray(cols[:, k]) for k in range(4))
        self._row = {}
        for i, n in enumerate(self.names):
            if n in self._row:
                raise ValueError("%s: the sequence name %r occurs twice" % (self.path, n))
            self._row[n] = i

    def __len__(self):
        return len(self.names)

    @property
    def records(self):
        """[(name, length, offset, line_bases, line_width)]: the lines of the .fai file"""
        return [(n, int(a), int(b), int(c), int(d)) for n, a, b, c, d in zip(self.names, self.length, self.offset, self.line_bases, self.line_width)]

    def _read_fai(self, fai):
        rec = []
        with open(fai) as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line:
                    continue
                cols = line.split("\t")
                try:
                    rec.append((cols[0],) + tuple(int(x) for x in cols[1:5]))
                    bad = len(rec[-1]) != 5 or min(rec[-1][1:]) < 0
                except ValueError:
                    bad = True
                if bad:
                    raise ValueError("%s line %d: name, length, offset, line bases and line width wanted, tab-separated" % (fai, no))
        mm = _map(self.path, self.size)
        for name, length, offset, lb, lw in rec:
            if length == 0:
                ok = offset <= self.size
            else:
                ok = lb > 0 and lw >= lb and 0 < offset <= self.size and mm[offset - 1] == 10 \
                    and offset + ((length - 1) // lb) * lw + (length - 1) % lb < self.size
            if not ok:
                raise ValueError("%s is stale: its record of sequence %r (length %d, offset %d, %d bases and %d bytes a line) does not fit %s "
                                 "(%d bytes); delete it or rebuild it" % (fai, name, length, offset, lb, lw, self.path, self.size))
        return rec

    def _scan(self):
        """the records from the file itself: the positions of the line ends, then everything by line, in numpy"""
        size = self.size
        if size == 0:
            return []
        mm = _map(self.path, size)
        ends = [np.flatnonzero(mm[p:p + _SCAN_BYTES] == 10) + p for p in range(0, size, _SCAN_BYTES)]
        end = np.concatenate(ends).astype(np.int64)                   # a line's '\n', or the file's size for a last line without one
        terminated = np.ones(end.size, bool)
        if mm[size - 1] != 10:
            end = np.append(end, size)
            terminated = np.append(terminated, False)
        start = np.empty_like(end)
        start[0] = 0
        start[1:] = end[:-1] + 1
        width = end - start + terminated                                # bytes of the line, its end included
        cr = (end > start) & (mm[np.maximum(end - 1, 0)] == 13)         # "\r\n" (or a "\r" before the end of the file)
        bases = end - start - cr
        header = (bases > 0) & (mm[np.minimum(start, size - 1)] == 62)
        h = np.flatnonzero(header)
        seq = np.cumsum(header) - 1                                     # the record a line belongs to
        stray = np.flatnonzero((seq < 0) & (bases > 0))
        if stray.size:
            raise ValueError("%s line %d: text before the first '>' header" % (self.path, stray[0] + 1))
        n = h.size
        body = np.flatnonzero(~header & (seq >= 0))                     # the sequence lines
        bseq, bb, bw = seq[body], bases[body], width[body]
        first = h + 1                                                   # a record's first sequence line, if it has one
        has = (first < end.size) & ~header[np.minimum(first, end.size - 1)]
        lb = np.where(has, bases[np.minimum(first, end.size - 1)], 0)
        lw = np.where(has, width[np.minimum(first, end.size - 1)], 0)
        last = np.full(n, -1, np.int64)                                 # a record's last line that holds bases
        np.maximum.at(last, bseq[bb > 0], body[bb > 0])
        inner = body < last[bseq]
        for bad in np.flatnonzero(inner & ((bb != lb[bseq]) | (bw != lw[bseq])))[:1]:
            name = self._name(mm, start[h[bseq[bad]]], end[h[bseq[bad]]])
            if bb[bad] == 0:
                raise ValueError("%s line %d: a blank line inside sequence %r" % (self.path, body[bad] + 1, name))
            raise ValueError("%s line %d: sequence %r has lines of different length (%d bases in %d bytes here, %d in %d in its first line)"
                             % (self.path, body[bad] + 1, name, bb[bad], bw[bad], lb[bseq[bad]], lw[bseq[bad]]))
        for bad in np.flatnonzero((body == last[bseq]) & (bb > lb[bseq]))[:1]:
            raise ValueError("%s line %d: the last line of sequence %r is longer than its first (%d bases, %d there)"
                             % (self.path, body[bad] + 1, self._name(mm, start[h[bseq[bad]]], end[h[bseq[bad]]]), bb[bad], lb[bseq[bad]]))
        length = np.zeros(n, np.int64)
        np.add.at(length, bseq, bb)
        offset = np.minimum(end[h] + 1, size)
        lb = np.where(length > 0, lb, 0)
        lw = np.where(length > 0, lw, 0)
        return [(self._name(mm, start[h[i]], end[h[i]]), int(length[i]), int(offset[i]), int(lb[i]), int(lw[i])) for i in range(n)]

    @staticmethod
    def _name(mm, start, end):
        text = bytes(mm[start + 1:end]).decode("latin-1").split()
        return text[0] if text else ""

    def write_fai(self, path=None):
        """the records as a .fai file (default: next to the FASTA file), as `samtools faidx` writes it"""
        with open(self.path + ".fai" if path is None else path, "w") as f:
            for r in self.records:
                f.write("%s\t%d\t%d\t%d\t%d\n" % r)

    def rows(self, name):
        """the record index of every name (a name or a sequence of names); ValueError for a name the file does not have"""
        names = [name] if isinstance(name, (str, bytes)) else list(name)
        try:
            return np.fromiter((self._row[str(n)] for n in names), dtype=np.int64, count=len(names))
        except KeyError as e:
            raise ValueError("sequence %s is not in %s" % (e, self.path)) from None

    def byte_range(self, name, start, end):
        """(first, last_excl), int64: the file bytes [first, last_excl) that hold the bases start .. end (1-based, both included) of sequence
        `name` -- scalars or arrays, a single name serves every range.  The address of the 0-based base p is
        offset + (p // line_bases) * line_width + p % line_bases.  The line ends between the first and the last base are inside the range on
        purpose: they are not letters, and the device counter counts letters.  ValueError: an unknown name, start < 1, end < start, end > length."""
        start = np.atleast_1d(np.asarray(start, dtype=np.int64))
        end = np.atleast_1d(np.asarray(end, dtype=np.int64))
        row = self.rows(name)
        if row.size == 1 and start.size != 1:
            row = np.repeat(row, start.size)
        if not (row.size == start.size == end.size):
            raise ValueError("name, start and end must have the same length")
        bad = np.flatnonzero((start < 1) | (end < start))
        if bad.size:
            raise ValueError("range %d is [%d, %d]: 1 <= start <= end wanted" % (bad[0], start[bad[0]], end[bad[0]]))
        bad = np.flatnonzero(end > self.length[row])
        if bad.size:
            raise ValueError("range %d ends at base %d, beyond the %d bases of sequence %r" % (bad[0], end[bad[0]], self.length[row[bad[0]]],
                                                                                            self.names[row[bad[0]]]))
        off, lb, lw = self.offset[row], self.line_bases[row], self.line_width[row]
        p, q = start - 1, end - 1
        return off + (p // lb) * lw + p % lb, off + (q // lb) * lw + q % lb + 1
