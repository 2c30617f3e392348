"""Not a test: the BGZF blocks that the inflate tests share (tests/test_inflate_host.py through tools/inflate_check.cpp, tests/test_gpu_bamdev.py
through ed_bamdev_*).  Python's zlib is the reference: a block must be accepted if and only if exomedepth_amd.bam._inflate returns, with its bytes.

  cases()        [(name, block, payload)]: well-formed blocks at the shapes where a decoder goes wrong
  bad_blocks()   [(name, block, status name or None)]: hand-made refusals, each refused by _inflate
  lane_cases()   ((name, block, payload), ...): blocks made by hand from ops (fixed_stream, dynamic_stream, stored_stream, join) at the edges of the
                 64-lane executor: pending literals x distance x length, dependent chains of matches, mixed block types in one BGZF block, code
                 tables zlib never writes, ISIZE at the edges of the CRC slices
  oversize_cases()  the one stored block too long for a BGZF block: for the host checkers only
  lane_bad_blocks() [(name, block, status name)]: refusals zlib's own output never comes near
  corruptions(b) every single-byte corruption of block b (all 255 other values of every byte): [(block, payload or None)] labelled by _inflate
  small_blocks() the three small blocks (stored, fixed, dynamic) whose corruptions are run
"""
import functools
import random
import struct
import zlib

from exomedepth_amd.bam import BGZF_EOF, _inflate

SIZES = (0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280)


def wrap(deflate, payload, crc=None, isize=None, oversize=False):
    """a BGZF block around a raw DEFLATE stream (oversize: more bytes than BSIZE can say -- no BGZF block any more, see oversize_cases)"""
    size = 18 + len(deflate) + 8
    assert size <= 65536 or oversize, size
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, (size - 1) & 0xFFFF) + deflate
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc, len(payload) if isize is None else isize))


def block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        d = c.compress(payload) + c.flush()
    else:
        d = c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    return wrap(d, payload)


def text(n, seed):
    """n bytes a compressor finds matches and skewed frequencies in"""
    r = random.Random(seed)
    words = [bytes(r.choices(b"ACGTNacgt0123456789:;=@", k=r.randint(2, 12))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) if r.random() < 0.8 else bytes([r.randrange(256)])
    return bytes(out[:n])


def noise(n, seed):
    return random.Random(seed).randbytes(n)


def fibonacci_payload():
    """byte frequencies 1, 1, 2, 3, 5, ...: an unrestricted Huffman code would be 21 bits deep, so zlib's length-limited one reaches 15"""
    f, out = [1, 1], bytearray()
    while sum(f) + f[-1] + f[-2] <= 65280:
        f.append(f[-1] + f[-2])
    for k, n in enumerate(f):
        out += bytes([65 + k]) * n
    random.Random(5).shuffle(out)
    return bytes(out)


class Bits:
    """a DEFLATE bit writer: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        if self.n >= 512:                # whole bytes go out 64 and more at a time: the lane lists put a million literals
            self._whole_bytes()

    def _whole_bytes(self):
        k = self.n >> 3
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    def align(self):
        """zero bits up to the next byte boundary: after it `out` holds everything (a stored block's bytes follow)"""
        self.n = (self.n + 7) & ~7
        self._whole_bytes()

    def code(self, value, bits):
        self.put(int(format(value, "0%db" % bits)[::-1], 2), bits)

    def fixed_literal(self, s):          # also the length symbols 256 .. 287
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def bytes(self):
        self._whole_bytes()
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _symbols(length, dist):
    """(length symbol - 257, extra value, extra bits, distance symbol, extra value, extra bits) of a match"""
    ls = 28 if length == 258 else max(k for k in range(28) if _LBASE[k] <= length)
    ds = max(k for k in range(30) if _DBASE[k] <= dist)
    return ls, length - _LBASE[ls], _LEXT[ls], ds, dist - _DBASE[ds], _DEXT[ds]


def _canonical(lens):
    """[(code bits reversed for Bits.put, length) or None] of the canonical Huffman code with these lengths (RFC 1951, 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(None)
            continue
        out.append((int(format(nxt[l], "0%db" % l)[::-1], 2), l))
        nxt[l] += 1
    return out


_FIXED_LIT = _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _canonical([5] * 32)


def _emit_coded(b, out, ops, lit, dist, end):
    """ops through the codes lit / dist onto the bit writer b, their bytes onto out.  An op is an int (a literal), a (length, distance) pair, or
    ("raw", value, bits): bits put as they are (for the refusals)"""
    for op in ops:
        if isinstance(op, int):
            b.put(*lit[op])
            out.append(op)
        elif op[0] == "raw":
            b.put(op[1], op[2])
        else:
            length, d = op
            ls, lv, lb, ds, dv, db = _symbols(length, d)
            b.put(*lit[257 + ls])
            b.put(lv, lb)
            b.put(*dist[ds])
            b.put(dv, db)
            for _ in range(length):
                out.append(out[-d] if d <= len(out) else 0)
    if end:
        b.put(*lit[256])


def _emit_fixed(b, out, ops, final=True, end=True):
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    _emit_coded(b, out, ops, _FIXED_LIT, _FIXED_DIST, end)


def rle(lens):
    """a length list as code-length symbols [(symbol, extra value)], greedily with the repeat symbols 16 (3 .. 6 of the last), 17 (3 .. 10 zeros)
    and 18 (11 .. 138 zeros)"""
    out, i = [], 0
    while i < len(lens):
        v, n = lens[i], 1
        while i + n < len(lens) and lens[i + n] == v:
            n += 1
        i += n
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11))
                n -= k
            if n >= 3:
                out.append((17, n - 3))
                n = 0
            out += [(0, 0)] * n
            continue
        out.append((v, 0))
        n -= 1
        while n >= 3:
            k = min(n, 6)
            out.append((16, k - 3))
            n -= k
        out += [(v, 0)] * n
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _emit_dynamic(b, out, lit_lens, dist_lens, ops, final=True, end=True, cl_syms=None):
    """cl_syms: None = every code length as itself (a code-length code of sixteen 4-bit codes); "rle" = rle() of the list (thirteen 4-bit and
    six 5-bit codes, so that 16, 17 and 18 have one); or the [(symbol, extra value)] list itself, which need not be a legal one"""
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(15, 4)                                   # all nineteen lengths of the code-length code
    if cl_syms is None:
        cl_lens = [4] * 16 + [0] * 3
        cl_syms = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    else:
        cl_lens = [4] * 13 + [5] * 6
        if isinstance(cl_syms, str):
            assert cl_syms == "rle"
            cl_syms = rle(list(lit_lens) + list(dist_lens))
    for s in _CL_ORDER:
        b.put(cl_lens[s], 3)
    cl = _canonical(cl_lens)
    for s, extra in cl_syms:
        b.put(*cl[s])
        if s >= 16:
            b.put(extra, _CL_EXTRA[s])
    _emit_coded(b, out, ops, _canonical(lit_lens), _canonical(dist_lens), end)


def _emit_stored(b, out, payload, final=True):
    assert len(payload) <= 65535
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(payload), 16)
    b.put(len(payload) ^ 0xFFFF, 16)
    b.align()
    b.out += payload
    out += payload


def fixed_stream(ops, final=True, end=True):
    """a fixed-Huffman DEFLATE block from ops: ints (literals) and (length, distance) pairs; returns (bytes, payload)"""
    b, out = Bits(), bytearray()
    _emit_fixed(b, out, ops, final, end)
    return b.bytes(), bytes(out)


def dynamic_stream(lit_lens, dist_lens, ops, final=True, end=True, cl_syms=None):
    """a dynamic-Huffman DEFLATE block: the code lengths of the literal / length symbols 0 .. len(lit_lens) - 1 and of the distance symbols, then ops
    through the canonical codes of those lengths; returns (bytes, payload).  cl_syms: see _emit_dynamic"""
    b, out = Bits(), bytearray()
    _emit_dynamic(b, out, lit_lens, dist_lens, ops, final, end, cl_syms)
    return b.bytes(), bytes(out)


def stored_stream(payload, final=True):
    b, out = Bits(), bytearray()
    _emit_stored(b, out, payload, final)
    return b.bytes(), bytes(out)


def join(*parts):
    """several DEFLATE blocks as one stream, bit after bit, all but the last with final = False; a match may reach back into the blocks before.
    A part is ("stored", payload), ("fixed", ops) or ("dynamic", lit_lens, dist_lens, ops[, cl_syms]); returns (bytes, payload)"""
    b, out = Bits(), bytearray()
    for k, part in enumerate(parts):
        final = k == len(parts) - 1
        if part[0] == "stored":
            _emit_stored(b, out, part[1], final)
        elif part[0] == "fixed":
            _emit_fixed(b, out, part[1], final)
        else:
            _emit_dynamic(b, out, part[1], part[2], part[3], final, True, part[4] if len(part) > 4 else None)
    return b.bytes(), bytes(out)


def flat_lens(symbols, size):
    """code lengths over `size` symbols: a complete code of the shortest near-equal lengths for `symbols` (one symbol: length 1), 0 elsewhere"""
    symbols = sorted(set(symbols))
    n = len(symbols)
    k = n.bit_length() - 1
    r = n - (1 << k)
    lens = [0] * size
    for j, s in enumerate(symbols):
        lens[s] = max(1, k if j < (1 << k) - r else k + 1)
    return lens


def far_repeat(dist):
    """literals, then a 258-byte match at exactly `dist` (zlib itself never reaches further back than 32 506)"""
    lits = list(noise(dist, 70 + dist % 7))
    d, payload = fixed_stream(lits + [(258, dist)])
    return wrap(d, payload), payload


def cases():
    out = []
    for n in SIZES:
        for level in (0, 1, 6, 9):
            p = noise(n, n) if level == 0 else text(n, n + level)
            out.append(("size %d level %d" % (n, level), block(p, level), p))
    assert len(out[36][1]) > 65280 and out[36][0] == "size 65280 level 0"          # one stored block of the largest payload still fits
    for name, strategy in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman-only", zlib.Z_HUFFMAN_ONLY)):
        for n in (1, 259, 32769):
            p = text(n, 11 * n)
            out.append(("%s %d" % (name, n), block(p, 6, strategy), p))
    p = bytes([7]) * 700 + text(300, 3) + bytes([9]) * 258 + bytes([1]) * 259
    out.append(("rle runs", block(p, 6, zlib.Z_RLE), p))
    out.append(("zeros", block(bytes(65280)), bytes(65280)))
    for period in (2, 3, 8):
        p = (b"ACGTTGCA"[:period] * 2000)[:3001]
        out.append(("period %d" % period, block(p, 9), p))
    for dist in (32768, 32767):
        b, p = far_repeat(dist)
        out.append(("repeat at distance %d" % dist, b, p))
    p = text(5000, 77)
    out.append(("full flush", block(p, 6, flush_at=2500), p))
    p = fibonacci_payload()
    out.append(("fibonacci huffman-only", block(p, 6, zlib.Z_HUFFMAN_ONLY), p))
    out.append(("eof block", BGZF_EOF, b""))
    p = text(3000, 8)
    b = block(p)
    out.append(("bytes after the final block", _resize(b[:-8] + b"\x55\xaa\x00" + b[-8:]), p))
    for name, b, p in out:
        assert _inflate(b) == p, name
    return out


def _resize(b):
    """the BC subfield's size word made right again after bytes were put into a block"""
    return b[:16] + struct.pack("<H", len(b) - 1) + b[18:]


def small_blocks():
    """stored, fixed, dynamic: at most 200 bytes compressed each"""
    p = text(60, 1)
    stored = block(p, 0)
    fixed = block(p, 6, zlib.Z_FIXED)
    q = bytes(random.Random(6).choices(b"ACGTNacgtn!#%&", weights=[30, 20, 15, 10, 8, 5, 4, 3, 2, 1, 1, 1, 1, 1], k=260))
    dynamic = block(q, 9)
    assert (dynamic[18] >> 1) & 3 == 2 and (fixed[18] >> 1) & 3 == 1 and (stored[18] >> 1) & 3 == 0
    assert max(len(stored), len(fixed), len(dynamic)) <= 200
    return [("stored", stored, p), ("fixed", fixed, p), ("dynamic", dynamic, q)]


def label(b):
    """what bam._inflate does with a block: its bytes, or None when it raises"""
    try:
        return _inflate(b)
    except Exception:
        return None


def corruptions(b):
    out = []
    for k in range(len(b)):
        for v in range(256):
            if v != b[k]:
                c = b[:k] + bytes([v]) + b[k + 1:]
                out.append((c, label(c)))
    return out


def bad_blocks():
    """hand-made refusals: (name, block, the status the decoder must name, or None where several are right)"""
    p = text(500, 21)
    good = block(p)
    out = [("flipped crc byte", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:], "BAD_CRC"),
           ("isize one less", good[:-4] + struct.pack("<I", len(p) - 1), "OUTPUT_OVERRUN"),
           ("isize one more", good[:-4] + struct.pack("<I", len(p) + 1), "SIZE_MISMATCH")]
    out.append(("block type 3", wrap(bytes([0b111]) + bytes(8), b""), "BAD_BTYPE"))
    out.append(("len / nlen mismatch", wrap(bytes([1]) + struct.pack("<HH", 5, 0xFFFA ^ 1) + b"hello", b"hello"), "BAD_STORED_LEN"))
    d = good[18:-8]
    out.append(("truncated stream", _resize(good[:18] + d[:len(d) // 2] + good[-8:]), None))
    d, _ = fixed_stream([65, 66, 67], end=False)
    out.append(("stream ends before the end-of-block symbol", wrap(d, b"ABC"), "INPUT_OVERRUN"))
    d, q = fixed_stream([65, 66, 67, (3, 4)])
    out.append(("distance before the start", wrap(d, q), "BAD_DISTANCE"))
    b = Bits()                                   # a dynamic block whose code-length code has three codes of length 1
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(0, 4)
    for _ in range(3):
        b.put(1, 3)
    b.put(0, 3)
    b.put(0, 32)
    out.append(("over-subscribed code-length code", wrap(b.bytes(), b""), "BAD_CODE_LENGTHS"))
    b = Bits()                                   # HLIT = 30: 287 literal/length codes
    b.put(1, 1); b.put(2, 2); b.put(30, 5); b.put(0, 5); b.put(15, 4)
    b.put(0, 64)
    out.append(("too many length codes", wrap(b.bytes(), b""), "BAD_CODE_LENGTHS"))
    b = Bits()
    b.put(1, 1); b.put(1, 2)
    b.fixed_literal(65)
    b.fixed_literal(286)
    b.put(0, 16)
    out.append(("length symbol 286", wrap(b.bytes(), b"A"), "BAD_SYMBOL"))
    b = Bits()
    b.put(1, 1); b.put(1, 2)
    b.fixed_literal(65)
    b.fixed_literal(257)
    b.code(30, 5)
    b.put(0, 16)
    out.append(("distance symbol 30", wrap(b.bytes(), b"A"), "BAD_SYMBOL"))
    out.append(("xlen reaching into the trailer", good[:10] + struct.pack("<H", len(good)) + good[12:], "BAD_HEADER"))
    for name, blk, _ in out:
        assert label(blk) is None, name
    return out


# ------------------------------------------------------------------------------------------------ where the lanes of the 64-lane executor share work
PENDING = (0, 1, 2, 62, 63, 64, 65, 127, 128, 129)
DISTANCES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 257, 258, 259)
LENGTHS = (3, 4, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 257, 258)
ISIZES = (3, 62, 63, 64, 65, 66, 127, 128, 129, 4032, 4095, 4096, 4097, 65535, 65536)
MAX_LANE_PAYLOAD = 60000
DENSE_LIT = flat_lens(range(286), 286)               # every literal / length symbol: 226 codes of 8 bits, 60 of 9
DENSE_DIST = flat_lens(range(30), 30)                # every distance symbol: 2 codes of 4 bits, 28 of 5
STAIRS = list(range(1, 16)) + [15]                   # a complete code with every length 1 .. 15


def triples():
    """(pending literals, distance, length): the product of the three lists, with distance also P and P + 1 (the match begins at the first pending
    literal, and one byte before it)"""
    out = []
    for p in PENDING:
        for d in sorted(set(DISTANCES) | {x for x in (p, p + 1) if x >= 1}):
            out += [(p, d, l) for l in LENGTHS]
    return out


def triple_ops(k, p, d, l):
    """261 noise literals, a match that flushes them, p noise literals, the match, a literal -- the noise is the case's own"""
    r = random.Random(1000 + k)
    return list(r.randbytes(261)) + [(3 + k % 5, 1 + k % 261)] + list(r.randbytes(p)) + [(l, d), r.randrange(256)]


def _packed(name, groups, coder):
    """groups of ops cut into blocks of at most MAX_LANE_PAYLOAD inflated bytes: coder(k)(ops) gives block k's (DEFLATE bytes, payload)"""
    out, ops, size = [], [], 0
    def close():
        d, payload = coder(len(out))(ops)
        out.append(("%s %d" % (name, len(out)), wrap(d, payload), payload))
    for g in groups:
        n = sum(1 if isinstance(op, int) else op[0] for op in g)
        if size + n > MAX_LANE_PAYLOAD:
            close()
            ops, size = [], 0
        ops += g
        size += n
    close()
    return out


def _fixed_or_dense(k):
    return fixed_stream if k % 2 == 0 else (lambda ops: dynamic_stream(DENSE_LIT, DENSE_DIST, ops))


def chain_groups(n, between, seed):
    """n matches back to back, dist == len, lengths cycling 3 .. 258: each reads what the one before it wrote (and, with `between`, the literal
    after it).  Each group opens with 258 literals of its own, so the groups can be cut into blocks anywhere"""
    r = random.Random(seed)
    groups, g, size = [], None, 0
    for k in range(n):
        l = 3 + k % 256
        if g is None or size + l + 1 > MAX_LANE_PAYLOAD // 2:
            g, size = list(r.randbytes(258)), 258
            groups.append(g)
        g.append((l, l))
        size += l
        if between:
            g.append(r.randrange(256))
            size += 1
    return groups


def _stairs_lit(symbols):
    """literal / length code lengths 1 .. 15, 15 on sixteen symbols (256 among them), the longest codes on the first"""
    assert len(symbols) == 16 and 256 in symbols
    lens = [0] * (max(symbols) + 1 if max(symbols) >= 257 else 257)
    for s, l in zip(symbols, STAIRS[::-1]):
        lens[s] = l
    return lens


@functools.lru_cache(maxsize=None)
def lane_cases():
    """((name, block, payload), ...): accepted blocks made by hand at the edges of the 64-lane executor, each labelled by _inflate.
    Made once a process: the tests that share it leave it as it is"""
    out = _packed("triples", [triple_ops(k, *t) for k, t in enumerate(triples())], _fixed_or_dense)
    out += _packed("chain", chain_groups(2000, False, 31), _fixed_or_dense)
    out += _packed("chain with a literal between", chain_groups(2000, True, 32), _fixed_or_dense)

    # ---- mixed block types in one BGZF block: n literals pending when each coded block ends, matches that reach back into stored bytes
    for n in (1, 63, 64, 65):
        r = random.Random(50 + n)
        s1, s2 = r.randbytes(300), r.randbytes(70)
        lits = lambda: list(r.randbytes(n))
        fixed = [(40, 300), (258, 259)] + lits()                                  # from the stored bytes; then n literals pending at the end
        dyn = [(5, n + 2), (64, n + 298 + 40)] + lits()                           # across the fixed block's pending literals, into the stored ones
        tail = [(65, n + 70), (3, 1)] + lits()                                    # across the last stored block
        d, p = join(("stored", s1), ("fixed", fixed), ("dynamic", DENSE_LIT, DENSE_DIST, dyn), ("stored", s2), ("fixed", tail))
        out.append(("stored fixed dynamic stored fixed, %d pending" % n, wrap(d, p), p))
        d, p = join(("fixed", lits()), ("stored", s2), ("dynamic", DENSE_LIT, DENSE_DIST, [(n + 3, n + 70)] + lits()), ("stored", b""),
                    ("fixed", lits()), ("fixed", []), ("stored", s1[:n]))
        out.append(("pending literals in front of stored blocks, %d" % n, wrap(d, p), p))
    for n in (0, 1, 63, 64, 65, 65505):                                           # (65 505: the longest stored block a BGZF block has room for)
        s = noise(n, 60 + n)
        d, p = stored_stream(s)
        out.append(("stored %d" % n, wrap(d, p), p))
        if n <= 65:
            d, p = join(("fixed", [1, 2, 3]), ("stored", s), ("fixed", [(3 + n, 3 + n)] if n else [4]), ("stored", s), ("stored", b""))
            out.append(("stored %d among coded blocks" % n, wrap(d, p), p))

    # ---- dynamic tables that zlib never writes
    lit = flat_lens([65, 66, 256, 257, 258, 285], 286)
    d, p = dynamic_stream(lit, [1], [65, 66, (3, 1), (4, 1), (258, 1), 66])
    out.append(("one distance code of length 1", wrap(d, p), p))
    d, p = dynamic_stream(flat_lens(list(range(256)) + [256], 257), [0], list(noise(200, 3)))
    out.append(("no distance code", wrap(d, p), p))
    d, p = dynamic_stream([0] * 256 + [1], [0], [])
    out.append(("end-of-block alone", wrap(d, p), p))
    d, p = dynamic_stream([0] * 256 + [1], [0], [], cl_syms="rle")
    out.append(("end-of-block alone, repeat symbols", wrap(d, p), p))
    r = random.Random(81)
    ops = list(r.randbytes(300)) + [(258, 300), (258, 245), (257, 2), 7, (258, 1)]
    d, p = dynamic_stream(DENSE_LIT, DENSE_DIST, ops + list(r.randbytes(25000)) + [(258, 24577), (3, 25000)])
    out.append(("HLIT 286 and HDIST 30, symbols 285 and 29 used", wrap(d, p), p))
    syms = [65, 66, 67, 68, 69, 70, 71, 72, 256, 257, 264, 265, 270, 280, 284, 285]
    lit = _stairs_lit(syms)
    ops = []
    for k in range(40):                                                           # every symbol of either code, the 15-bit ones among them
        ops += [65 + k % 8, (_LBASE[(257, 264, 265, 270, 280, 284, 285)[k % 7] - 257], _DBASE[k % 16] if _DBASE[k % 16] <= 8 * (k + 1) else 1)] + [72, 71] * 4
    for cl_syms in (None, "rle"):
        d, p = dynamic_stream(lit, STAIRS, ops, cl_syms=cl_syms)
        out.append(("all fifteen code lengths in both codes%s" % (", repeat symbols" if cl_syms else ""), wrap(d, p), p))
    # runs of repeat symbols that stop exactly at the end of the literal lengths; one that crosses from the literal into the distance lengths; one
    # that ends exactly at nlen + ndist
    d, p = dynamic_stream([8] * 252 + [9] * 8, [5] * 28 + [4] * 2, [0, 1, (3, 2), 251, (5, 1), (4, 3)], cl_syms="rle")
    out.append(("repeat runs that stop at the end of the literal lengths", wrap(d, p), p))
    lit, dist = [3] * 4 + [0] * 252 + [2, 2], [2] * 4 + [0] * 26
    syms = [(3, 0), (16, 0), (18, 127), (18, 103), (2, 0), (16, 2), (18, 15)]     # 3 x 4, 138 + 114 zeros, 2 x 6 (two of them literal lengths), 26 zeros
    assert sum(1 if s < 16 else e + (3 if s < 18 else 11) for s, e in syms) == len(lit) + len(dist)
    d, p = dynamic_stream(lit, dist, [0, 1, 2, 3, (3, 4), (3, 1), (3, 2), (3, 3)], cl_syms=syms)
    out.append(("a repeat run across the literal / distance border, another to exactly nlen + ndist", wrap(d, p), p))

    # ---- ISIZE at the edges of the CRC slices (ceil(ISIZE / 64) bytes a lane, empty slices at the top)
    for n in ISIZES:
        for level in (0, 6):
            t = text(n, 5)
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = c.compress(t) + c.flush()
            if 18 + len(d) + 8 <= 65536:
                out.append(("isize %d level %d" % (n, level), wrap(d, t), t))
    for name, b, p in out:
        assert len(b) <= 65536 and _inflate(b) == p, name
    return tuple(out)


def oversize_cases():
    """[(name, bytes, payload)] for the host checkers alone: a stored block of 65 535 bytes is 30 bytes more than a BGZF block holds (BSIZE is 16
    bits), so the device route, which cuts a file by BSIZE, can never be handed one; the decoder itself reads only XLEN and the trailer"""
    d, p = stored_stream(noise(65535, 9))
    b = wrap(d, p, oversize=True)
    assert _inflate(b) == p
    return [("stored 65535", b, p)]


def lane_bad_blocks():
    """[(name, block, status name)]: refusals made by hand, each refused by _inflate"""
    out = []
    lit = flat_lens([65, 256, 257], 258)
    d, _ = dynamic_stream(lit, [1], [65, 65, 65] + [("raw", _canonical(lit)[257][0], _canonical(lit)[257][1]), ("raw", 1, 1)] + [("raw", 0, 32)], end=False)
    out.append(("the unused pattern of a one-code distance code", wrap(d, b"AAA"), "BAD_SYMBOL"))
    lit = [0] * 258
    lit[65], lit[256] = 2, 2
    d, _ = dynamic_stream(lit, [0], [65])
    out.append(("incomplete literal code, codes of length 2", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    lit = [0] * 258
    lit[65], lit[256] = 1, 2
    d, _ = dynamic_stream(lit, [0], [65])
    out.append(("incomplete literal code, lengths 1 and 2", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    lit = flat_lens([65, 256], 257)
    d, _ = dynamic_stream(lit, [2, 2], [65])
    out.append(("incomplete distance code, codes of length 2", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    d, _ = dynamic_stream(lit, [0], [65], cl_syms=[(16, 0)] + rle(lit[3:] + [0]))
    out.append(("symbol 16 first in the length list", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    d, _ = dynamic_stream(lit, [0], [65], cl_syms=rle(lit) + [(17, 0)])
    out.append(("a repeat of zeros past nlen + ndist", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    d, _ = dynamic_stream(lit, [1], [65], cl_syms=rle(lit[:256]) + [(1, 0), (16, 0)])
    out.append(("a repeat of the last length past nlen + ndist", wrap(d, b"A"), "BAD_CODE_LENGTHS"))
    lit = flat_lens([65, 66], 257)
    d, _ = dynamic_stream(lit, [0], [65, 66], end=False)
    out.append(("no code for symbol 256", wrap(d, b"AB"), "BAD_CODE_LENGTHS"))
    for n in (1, 63, 64):
        r = random.Random(90 + n)
        head = list(r.randbytes(5)) + [(3, 1)]
        ops = head + list(r.randbytes(n)) + [(3, 8 + n + 1)]
        for name, coder in (("fixed", fixed_stream), ("dynamic", lambda ops: dynamic_stream(DENSE_LIT, DENSE_DIST, ops))):
            d, p = coder(ops)
            out.append(("distance pos + 1 with %d literals pending, %s" % (n, name), wrap(d, p), "BAD_DISTANCE"))
            d, p = coder(list(r.randbytes(300)) + [(9, 300)] + list(r.randbytes(n)) + [66])
            out.append(("a literal one byte past isize, after %d literals, %s" % (n, name), wrap(d, p[:-1]), "OUTPUT_OVERRUN"))
            d, p = coder(list(r.randbytes(300)) + [(9, 300)] + list(r.randbytes(n)) + [(70, 5)])
            out.append(("a match one byte past isize, %d pending, %s" % (n, name), wrap(d, p[:-1]), "OUTPUT_OVERRUN"))
    for name, blk, _ in out:
        assert label(blk) is None, name
    return out
