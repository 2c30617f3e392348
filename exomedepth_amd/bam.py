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


INFLATE_STATUS = ("OK", "BAD_HEADER", "BAD_BTYPE", "BAD_STORED_LEN", "BAD_CODE_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE", "OUTPUT_OVERRUN",
                  "INPUT_OVERRUN", "SIZE_MISMATCH", "BAD_CRC")


def bamdev_geometry():
    """{blocks_per_workgroup, threads, lds_bytes_per_block} of k_bgzf_inflate and the scan's blocks per workgroup (ed_bamdev_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_bamdev_geometry(out))
    return dict(zip(("blocks_per_workgroup", "threads", "lds_bytes_per_block", "scan_blocks_per_workgroup"), (int(v) for v in out)))


class DeviceInflater:
    """BGZF blocks inflated on the device (ed_bamdev, csrc/edinflate.inc): push() pieces of a file, end() it; after either, statuses() and
    inflated() give the last batch waited for.  A block that does not inflate fails the call that waits for its batch (EdError, ED_ERR_INVALID)."""

    def __init__(self, device=0, batch_bytes=32 << 20):
        self.handle = C.c_void_p()
        check(lib().ed_bamdev_create(C.byref(self.handle), int(device), int(batch_bytes)))

    def close(self):
        if self.handle:
            lib().ed_bamdev_destroy(self.handle)
            self.handle = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def begin(self, first_record_offset=-1, gap=0):
        """a new file.  first_record_offset: the length of the BAM header in the inflated stream = scan and gather every batch's records on the
        device; -1 = inflate only.  gap (tests): guard bytes around every block's output slot, no scan"""
        check(lib().ed_bamdev_begin(self.handle, int(first_record_offset)))
        if gap:
            check(lib().ed_bamdev_set_guard_gap(self.handle, int(gap)))
        self.n_records = 0

    def push(self, buf):
        """takes the whole BGZF blocks at the front of buf (at most a batch of them); returns the bytes taken"""
        a = np.frombuffer(buf, dtype=np.uint8)
        used, n = C.c_int64(0), C.c_int64(0)
        self.n_records = 0
        check(lib().ed_bamdev_push(self.handle, C.c_void_p(a.ctypes.data) if a.size else None, a.size, C.byref(used), C.byref(n)))
        self.n_records = n.value                         # records of the batch this push waited for
        return used.value

    def records(self):
        """the records of the last batch waited for, on the device (DeviceRecords)"""
        n, ptrs = C.c_int64(0), (C.c_void_p * 4)()
        check(lib().ed_bamdev_records(self.handle, C.byref(n), ptrs))
        return DeviceRecords(self, n.value, [p or 0 for p in ptrs])

    def end(self):
        check(lib().ed_bamdev_end(self.handle))

    def statuses(self):
        n = C.c_int64(0)
        check(lib().ed_bamdev_block_status(self.handle, 0, None, C.byref(n)))
        out = np.empty(n.value, np.int32)
        check(lib().ed_bamdev_block_status(self.handle, out.size, C.c_void_p(out.ctypes.data) if out.size else None, C.byref(n)))
        return out

    def inflated(self):
        """the last batch's inflated bytes (with the guard bytes of begin(gap) where they lie)"""
        n = C.c_int64(0)
        lib().ed_bamdev_copy_inflated(self.handle, None, 0, C.byref(n))           # (fails for want of room, and says how much)
        out = np.empty(n.value, np.uint8)
        check(lib().ed_bamdev_copy_inflated(self.handle, C.c_void_p(out.ctypes.data) if out.size else None, out.size, C.byref(n)))
        return out

    def kernel_ms(self):
        """(inflate, scan, gather) device milliseconds so far"""
        a = (C.c_double * 3)()
        check(lib().ed_bamdev_kernel_ms(self.handle, a))
        return tuple(a)


class DeviceRecords:
    """one batch's records on the device: n, and ptrs = the device addresses of refid, pos, tlen (int32) and flag_mapq (uint32).  They stand until
    the second push after the one that returned them (owner: the DeviceInflater, kept alive here)."""

    def __init__(self, owner, n, ptrs):
        self.owner, self.n, self.ptrs = owner, int(n), tuple(ptrs)

    def to_host(self):
        out = tuple(np.empty(self.n, dt) for dt in _DTYPES)
        for o, p in zip(out, self.ptrs):
            if self.n:
                check(lib().ed_memcpy_d2h(C.c_void_p(o.ctypes.data), C.c_void_p(p), o.nbytes))
        return out


class DeviceBamFile:
    """Header and records of one BAM file by the device route: the header is read on the host from the first blocks (BamFile's parser), then the
    whole file crosses the link compressed and batches() yields a DeviceRecords per batch -- inflated, CRC-checked, scanned and gathered on the
    device.  The same errors for the same files as BamFile (ValueError)."""

    def __init__(self, path, device=0, batch_bytes=32 << 20):
        self.path = os.fspath(path)
        with BamFile(self.path, batch_bytes=min(int(batch_bytes), 1 << 20)) as b:
            self.text, self.ref_names, self.ref_lengths, self.first_record_offset = b.text, b.ref_names, b.ref_lengths, b.first_record_offset
        self.device, self.batch_bytes = int(device), int(batch_bytes)
        self.kernel_ms = (0.0, 0.0, 0.0)

    def batches(self):
        from ._lib import EdError
        with DeviceInflater(self.device, self.batch_bytes) as d, open(self.path, "rb") as f:
            d.begin(self.first_record_offset)
            tail, at, n_blocks = b"", 0, 0
            try:
                while True:
                    piece = f.read(self.batch_bytes)
                    buf = tail + piece
                    off = 0
                    while True:
                        size = _block_size(buf, off)
                        if size is None or len(buf) - off < size:
                            break
                        used = d.push(memoryview(buf)[off:])
                        if d.n_records:
                            yield d.records()
                        n_blocks += used > 0
                        off += used
                    tail = buf[off:]
                    at += off
                    if not piece:
                        break
                if tail:
                    raise ValueError("truncated BGZF file: %d bytes after the last whole block (at byte %d)" % (len(tail), at))
                if n_blocks == 0:
                    raise ValueError("not a BGZF file: it is empty")
                try:
                    d.end()
                finally:
                    rec = d.records()                    # the last batch's, also when the stream ends inside a record
                    self.kernel_ms = d.kernel_ms()
                if rec.n:
                    yield rec
            except EdError as e:
                if any(k in str(e) for k in ("corrupt BGZF block", "not a BGZF file", "truncated BAM")):
                    raise ValueError(str(e).split("libedcore: ")[-1]) from None
                if "block_size" in str(e):               # a bad record (EdError, as from the host scanner): the records before it are delivered
                    rec = d.records()
                    if rec.n:
                        yield rec
                raise

    def records(self):
        """all records of the file as four host arrays (small files, tests)"""
        got = [r.to_host() for r in self.batches()]
        return tuple(np.concatenate([g[k] for g in got]) if got else np.empty(0, _DTYPES[k]) for k in range(4))


def _inflated_device(path, device, batch_bytes):
    """inflated() by the device route: the same pieces, the same errors for the same files (a block that does not inflate: ValueError)"""
    from ._lib import EdError
    with DeviceInflater(device, batch_bytes) as d, open(path, "rb") as f:
        d.begin()
        tail, at, n_blocks, pending = b"", 0, 0, False
        try:
            while True:
                piece = f.read(batch_bytes)
                buf = tail + piece
                off = 0
                while True:                               # a piece may hold more than a batch of blocks
                    size = _block_size(buf, off)
                    if size is None or len(buf) - off < size:
                        break
                    used = d.push(memoryview(buf)[off:])  # waits for the batch before: its bytes can be fetched now
                    if pending:
                        yield d.inflated().tobytes()
                    pending = used > 0
                    n_blocks += used > 0
                    off += used
                tail = buf[off:]
                at += off
                if not piece:
                    break
            d.end()
            if pending:
                yield d.inflated().tobytes()
        except EdError as e:
            if "corrupt BGZF block" in str(e) or "not a BGZF file" in str(e):
                raise ValueError(str(e).split("libedcore: ")[-1]) from None
            raise
        if tail:
            raise ValueError("truncated BGZF file: %d bytes after the last whole block (at byte %d)" % (len(tail), at))
        if n_blocks == 0:
            raise ValueError("not a BGZF file: it is empty")


def inflated(path, pool=None, batch_bytes=32 << 20, device=None):
    """the inflated stream of a BGZF file, as a generator of bytes pieces (one per batch of about batch_bytes compressed bytes).
    device: None = inflate on the host's thread pool; a device number = the file crosses the link compressed and is inflated there
    (DeviceInflater), the pieces coming back for the host scanner."""
    if device is not None:
        yield from _inflated_device(path, int(device), int(batch_bytes))
        return
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
    batch_bytes: compressed bytes read and inflated per piece (a small value when only the header is wanted).
    device: None = inflate on the host; a device number = the blocks are inflated on that device (the records are scanned on the host either way)."""

    def __init__(self, path, pool=None, batch_bytes=32 << 20, device=None):
        self.path = os.fspath(path)
        self._own_pool = pool is None and device is None
        self._pool = ThreadPoolExecutor(n_threads()) if self._own_pool else pool
        self._pieces = inflated(self.path, self._pool, batch_bytes, device=device)     # device: a device number = inflate there (DeviceInflater)
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
        self.first_record_offset = off                        # where the records begin in the inflated stream
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
