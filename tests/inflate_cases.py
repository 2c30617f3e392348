"""Not a test: the BGZF blocks that the inflate tests share (tests/test_inflate_host.py through tools/inflate_check.cpp, tests/test_gpu_bamdev.py
through ed_bamdev_*).  Python's zlib is the reference: a block must be accepted if and only if exomedepth_amd.bam._inflate returns, with its bytes.

  cases()        [(name, block, payload)]: well-formed blocks at the shapes where a decoder goes wrong
  bad_blocks()   [(name, block, status name or None)]: hand-made refusals, each refused by _inflate
  corruptions(b) every single-byte corruption of block b (all 255 other values of every byte): [(block, payload or None)] labelled by _inflate
  small_blocks() the three small blocks (stored, fixed, dynamic) whose corruptions are run
"""
import random
import struct
import zlib

from exomedepth_amd.bam import BGZF_EOF, _inflate

SIZES = (0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280)


def wrap(deflate, payload, crc=None, isize=None):
    """a BGZF block around a raw DEFLATE stream"""
    size = 18 + len(deflate) + 8
    assert size <= 65536, size
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, size - 1) + deflate
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
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

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
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def fixed_stream(ops, final=True, end=True):
    """a fixed-Huffman DEFLATE block from ops: ints (literals) and (length, distance) pairs; returns (bytes, payload)"""
    b, out = Bits(), bytearray()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for op in ops:
        if isinstance(op, int):
            b.fixed_literal(op)
            out.append(op)
            continue
        length, dist = op
        ls = max(k for k in range(29) if _LBASE[k] <= length and (k < 28 or length == 258))
        if length == 258:
            ls = 28
        b.fixed_literal(257 + ls)
        b.put(length - _LBASE[ls], _LEXT[ls])
        ds = max(k for k in range(30) if _DBASE[k] <= dist)
        b.code(ds, 5)
        b.put(dist - _DBASE[ds], _DEXT[ds])
        for _ in range(length):
            out.append(out[-dist] if dist <= len(out) else 0)
    if end:
        b.fixed_literal(256)
    return b.bytes(), bytes(out)


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
