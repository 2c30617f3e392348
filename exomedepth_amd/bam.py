"""BAM files to record fields, with the standard library and numpy only (no pysam, no samtools).

A BAM file is a series of BGZF blocks -- gzip members of at most 64 KiB whose extra field names their own size -- which inflate to one
stream: the header (magic, SAM text, reference names and lengths), then the alignment records.  The blocks are inflated on a thread pool
(zlib releases the GIL); the record stream goes in chunks to the library's host scanner (ed_bam_scan_records, csrc/ed_bamscan.hpp), which
follows the records' block_size chain and copies out refID, pos, tlen and flag | mapq << 16 -- all the read counter looks at.  The whole file
is scanned: no index is read (the counts are the same).
"""
import ctypes as C
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._lib import check, lib

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the 28-byte empty block that ends a file
FIELDS = ("refid", "pos", "tlen", "flag_mapq")
_DTYPES = (np.int32, np.int32, np.int32, np.uint32)


def n_threads():
    """threads of the inflating pool: OMP_NUM_THREADS when set, else at most 16 -- never the machine's raw CPU count"""
    v = os.environ.get("OMP_NUM_THREADS", "").strip()
    if v.isdigit() and int(v) > 0:
        return int(v)
    return max(1, min(16, os.cpu_count() or 1))


def _block_size(buf, off):
    """total size of the BGZF block whose gzip header starts at buf[off], or None when the header is not wholly inside buf"""
    if len(buf) - off < 12:
        return None
    id1, id2, cm, flg, xlen = buf[off], buf[off + 1], buf[off + 2], buf[off + 3], buf[off + 10] | (buf[off + 11] << 8)
    if id1 != 31 or id2 != 139 or cm != 8 or not (flg & 4):
        raise ValueError("not a BGZF file: no gzip member with an extra field at byte %d" % off)
    if len(buf) - off < 12 + xlen:
        return None
    p, end = off + 12, off + 12 + xlen
    while p + 4 <= end:                                   # the extra field's subfields: SI1 SI2 SLEN data
        slen = buf[p + 2] | (buf[p + 3] << 8)
        if buf[p] == 66 and buf[p + 1] == 67 and slen == 2 and p + 6 <= end:
            size = (buf[p + 4] | (buf[p + 5] << 8)) + 1
            if size < 12 + xlen + 8:
                raise ValueError("not a BGZF file: block at byte %d names a size of %d" % (off, size))
            return size
        p += 4 + slen
    raise ValueError("not a BGZF file: the gzip member at byte %d has no BC subfield" % off)


def _inflate(block):
    xlen = block[10] | (block[11] << 8)
    data = zlib.decompress(block[12 + xlen:-8], -15)
    crc, isize = struct.unpack_from("<II", block, len(block) - 8)
    if len(data) != isize or (zlib.crc32(data) & 0xFFFFFFFF) != crc:
        raise ValueError("corrupt BGZF block: length or CRC-32 of the inflated data does not match its trailer")
    return data


def inflated(path, pool=None, batch_bytes=32 << 20):
    """the inflated stream of a BGZF file, as a generator of bytes pieces (one per batch of about batch_bytes compressed bytes)"""
    own = pool is None
    if own:
        pool = ThreadPoolExecutor(n_threads())
    try:
        with open(path, "rb") as f:
            tail, at, n_blocks = b"", 0, 0
            while True:
                piece = f.read(batch_bytes)
                buf = tail + piece
                blocks, off = [], 0
                while True:
                    size = _block_size(buf, off)
                    if size is None or len(buf) - off < size:
                        break
                    blocks.append(buf[off:off + size])
                    off += size
                tail = buf[off:]
                at += off
                n_blocks += len(blocks)
                if blocks:
                    yield b"".join(pool.map(_inflate, blocks))
                if not piece:
                    break
            if tail:
                raise ValueError("truncated BGZF file: %d bytes after the last whole block (at byte %d)" % (len(tail), at))
            if n_blocks == 0:
                raise ValueError("not a BGZF file: it is empty")
    finally:
        if own:
            pool.shutdown()


def scan_records(buf, cap=None):
    """ed_bam_scan_records on a bytes-like piece of the record stream: ((refid, pos, tlen, flag_mapq), bytes_consumed)"""
    a = np.frombuffer(buf, dtype=np.uint8)
    if cap is None:
        cap = a.size // 36 + 1                            # a record is at least 4 + 32 bytes
    out = [np.empty(cap, dt) for dt in _DTYPES]
    n, used = C.c_int64(0), C.c_int64(0)
    check(lib().ed_bam_scan_records(C.c_void_p(a.ctypes.data) if a.size else None, a.size, cap, *(C.c_void_p(o.ctypes.data) for o in out),
                                    C.byref(n), C.byref(used)))
    return tuple(o[:n.value] for o in out), used.value


def scan_stream(pieces):
    """records of a record stream that arrives in pieces (any sizes): a generator of (refid, pos, tlen, flag_mapq) per piece that completed a
    record.  A piece ends anywhere; what the scanner did not consume is carried into the next.  Bytes left at the end: ValueError."""
    tail = b""
    for piece in pieces:
        buf = tail + piece if tail else piece
        rec, used = scan_records(buf)
        tail = bytes(buf[used:])
        if rec[0].size:
            yield rec
    if tail:
        raise ValueError("truncated BAM: %d bytes of an incomplete record at the end of the stream" % len(tail))


class BamFile:
    """Header and records of one BAM file.  text, ref_names, ref_lengths are read on opening; chunks() then yields the records.
    pool: a ThreadPoolExecutor to inflate on (the caller's, shared between files); None = one of its own, n_threads() wide.
    batch_bytes: compressed bytes read and inflated per piece (a small value when only the header is wanted)."""

    def __init__(self, path, pool=None, batch_bytes=32 << 20):
        self.path = os.fspath(path)
        self._own_pool = pool is None
        self._pool = ThreadPoolExecutor(n_threads()) if pool is None else pool
        self._pieces = inflated(self.path, self._pool, batch_bytes)
        self._buf = b""
        try:
            self._read_header()
        except Exception:
            self.close()
            raise

    def _need(self, n):
        """at least n bytes in the buffer, or ValueError"""
        while len(self._buf) < n:
            try:
                self._buf += next(self._pieces)
            except StopIteration:
                raise ValueError("truncated BAM: the header of %s ends after %d bytes" % (self.path, len(self._buf)))

    def _read_header(self):
        self._need(4)
        if self._buf[:4] != b"BAM\1":
            raise ValueError("not a BAM file: %s starts with %r, not 'BAM\\1'" % (self.path, self._buf[:4]))
        self._need(8)
        l_text = struct.unpack_from("<i", self._buf, 4)[0]
        if l_text < 0:
            raise ValueError("corrupt BAM header: l_text = %d" % l_text)
        self._need(12 + l_text)
        self.text = self._buf[8:8 + l_text].split(b"\0")[0].decode(errors="replace")
        n_ref = struct.unpack_from("<i", self._buf, 8 + l_text)[0]
        if n_ref < 0:
            raise ValueError("corrupt BAM header: n_ref = %d" % n_ref)
        off = 12 + l_text
        self.ref_names, self.ref_lengths = [], []
        for _ in range(n_ref):
            self._need(off + 4)
            l_name = struct.unpack_from("<i", self._buf, off)[0]
            if l_name < 1:
                raise ValueError("corrupt BAM header: l_name = %d" % l_name)
            self._need(off + 8 + l_name)
            self.ref_names.append(self._buf[off + 4:off + 4 + l_name].split(b"\0")[0].decode(errors="replace"))
            self.ref_lengths.append(struct.unpack_from("<i", self._buf, off + 4 + l_name)[0])
            off += 8 + l_name
        self._buf = self._buf[off:]

    def chunks(self):
        """the records, once: a generator of (refid, pos, tlen, flag_mapq) arrays, one tuple per inflated batch"""
        def pieces():
            first, self._buf = self._buf, b""
            yield first
            yield from self._pieces
        try:
            yield from scan_stream(pieces())
        finally:
            self.close()

    def records(self):
        """all records of the file as four arrays (small files, tests)"""
        got = list(self.chunks())
        return tuple(np.concatenate([g[k] for g in got]) if got else np.empty(0, _DTYPES[k]) for k in range(4))

    def close(self):
        self._pieces.close()
        if self._own_pool and self._pool is not None:
            self._pool.shutdown()
        self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
