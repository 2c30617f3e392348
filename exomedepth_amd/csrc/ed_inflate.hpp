// ed_inflate.hpp -- the rules of inflating one BGZF block (RFC 1951 DEFLATE inside a gzip member, SAM specification section 4.1), written once
// for the host and for the device.  No HIP include and nothing of the library's: gcc compiles it as it is (tools/inflate_check.cpp runs it under
// the host sanitizers), hipcc compiles the same text for gfx950 (edinflate.inc, k_bgzf_inflate).  DESIGN 4.25.
//
// Acceptance rule: inflate_block gives OK if and only if exomedepth_amd.bam._inflate(block) returns, and then the bytes are equal -- i.e. what
// zlib's inflate (raw, 32 KiB window) accepts and the block's own CRC-32 and ISIZE confirm.  Like _inflate it reads of the gzip header only XLEN,
// and ignores what follows the final DEFLATE block.
//
// The decoder is a template over its executor W: Serial (one thread; the plain inflate_block below) or Lanes<P> (the kernel's 64 lanes of a
// wavefront; tools/inflate_lanes_check.cpp's emulated ones).  The symbol
// loop is the same for every lane of an executor; what the lanes share out is marked by loops of the form
//   for (i = w.lane(); i < n; i += w.lanes())
// and a w.sync() stands wherever a lane reads what another lane wrote (nothing for Serial).  Every loop consumes at least one input bit or one
// output byte per iteration or leaves with a status, so a corrupt block costs at most its own length in work.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ED_INF_HD __host__ __device__ inline
#else
#define ED_INF_HD inline
#endif

namespace edinf {

enum Status : int32_t {
  OK = 0,
  BAD_HEADER,          // shorter than header + trailer, or XLEN reaches into the trailer
  BAD_BTYPE,           // block type 3
  BAD_STORED_LEN,      // LEN != ~NLEN
  BAD_CODE_LENGTHS,    // HLIT / HDIST too large, a repeat with nothing before it or past the end, an over-subscribed or incomplete code, no symbol 256
  BAD_SYMBOL,          // a bit pattern that is no code, or literal/length symbol 286 / 287, or distance symbol 30 / 31
  BAD_DISTANCE,        // a distance reaching before the block's first output byte
  OUTPUT_OVERRUN,      // more than ISIZE bytes
  INPUT_OVERRUN,       // the DEFLATE data ended inside a symbol
  SIZE_MISMATCH,       // the final block ended with fewer than ISIZE bytes
  BAD_CRC,
  kNStatus
};

inline const char* status_name(int s)
{
  static const char* const names[kNStatus] = {"OK", "BAD_HEADER", "BAD_BTYPE", "BAD_STORED_LEN", "BAD_CODE_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE",
                                              "OUTPUT_OVERRUN", "INPUT_OVERRUN", "SIZE_MISMATCH", "BAD_CRC"};
  return (s >= 0 && s < kNStatus) ? names[s] : "?";
}

constexpr uint32_t kMaxInflated = 65536;     // what a BGZF block may hold (SAM specification 4.1); the device route refuses a larger ISIZE

ED_INF_HD uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
ED_INF_HD uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// ---------------------------------------------------------------------------------------------- the BGZF block
// Total size of the BGZF block whose gzip header starts at buf[0], by the rules of bam._block_size: 0 when the header is not wholly inside
// buf[0, n) (more bytes are needed), -1 when it is no BGZF header (magic, CM, FLG.FEXTRA, a BC subfield of length 2, a size that holds the header
// and the trailer).
ED_INF_HD int32_t bgzf_block_size(const uint8_t* buf, int64_t n)
{
  if (n < 12) return 0;
  if (buf[0] != 31 || buf[1] != 139 || buf[2] != 8 || !(buf[3] & 4)) return -1;
  const int64_t xlen = le16(buf + 10);
  if (n < 12 + xlen) return 0;
  int64_t p = 12;
  const int64_t end = 12 + xlen;
  while (p + 4 <= end) {
    const int64_t slen = le16(buf + p + 2);
    if (buf[p] == 66 && buf[p + 1] == 67 && slen == 2 && p + 6 <= end) {
      const int32_t size = (int32_t)le16(buf + p + 4) + 1;
      return size < 12 + xlen + 8 ? -1 : size;
    }
    p += 4 + slen;
  }
  return -1;
}

struct BlockInfo { uint32_t data_off, data_len, crc, isize; };

// Where the DEFLATE data of a whole block lies, and its trailer, by the rules of bam._inflate: XLEN alone says where the data begins.
ED_INF_HD int block_info(const uint8_t* block, uint32_t size, BlockInfo* bi)
{
  if (size < 12 + 8) return BAD_HEADER;
  const uint32_t xlen = le16(block + 10);
  if (12 + xlen > size - 8) return BAD_HEADER;
  bi->data_off = 12 + xlen;
  bi->data_len = size - 8 - bi->data_off;
  bi->crc = le32(block + size - 8);
  bi->isize = le32(block + size - 4);
  return OK;
}

// ---------------------------------------------------------------------------------------------- bits
// LSB-first bits of data[0, n).  peek() pads with zeros past the end; drop() of more bits than the data holds sets `over` for good (and empties the
// reader).  No byte outside [data, data + n) is read.
struct BitReader {
  const uint8_t* data;
  uint32_t n, pos;       // bytes; pos = next byte to load
  uint32_t cnt;          // valid bits in hold
  uint64_t hold;
  int32_t over;

  ED_INF_HD void init(const uint8_t* d, uint32_t len) { data = d; n = len; pos = 0; cnt = 0; hold = 0; over = 0; }
  ED_INF_HD void refill()
  {
    while (cnt <= 56 && pos < n) { hold |= (uint64_t)data[pos++] << cnt; cnt += 8; }
  }
  ED_INF_HD uint32_t peek(uint32_t k) { refill(); return (uint32_t)hold & ((1u << k) - 1u); }     // k <= 16
  ED_INF_HD void drop(uint32_t k)
  {
    if (k > cnt) { over = 1; cnt = 0; hold = 0; pos = n; }
    else { hold >>= k; cnt -= k; }
  }
  ED_INF_HD uint32_t get(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }
  ED_INF_HD uint32_t avail() { refill(); return cnt; }
  ED_INF_HD void align() { drop(cnt & 7u); }                                  // cnt = 8 * bytes loaded - bits consumed
  ED_INF_HD uint32_t byte_pos() const { return pos - (cnt >> 3); }            // after align(): the next unconsumed byte
  ED_INF_HD void seek(uint32_t p) { pos = p < n ? p : n; cnt = 0; hold = 0; }
};

// ---------------------------------------------------------------------------------------------- canonical Huffman codes
// A primary table of PB bits -- fast[bits] = length << 12 | symbol, 0 where no code of at most PB bits matches -- and, for longer codes, the
// canonical walk over count[] / sym[] (first code of every length, as in zlib's contrib/puff).
template <int PB, int NSYM>
struct Huff {
  static constexpr int kPrimaryBits = PB;
  uint16_t fast[1 << PB];
  uint16_t count[16];        // codes of each length; count[0] = symbols without a code
  uint16_t sym[NSYM];        // symbols in canonical order
};

ED_INF_HD uint32_t bit_reverse(uint32_t v, int n)
{
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
  return r;
}

// Tables of the code with lengths lens[0, n) (n <= NSYM, every length <= 15).  Returns < 0 for an over-subscribed code (the tables are then
// not filled), 0 for a complete one, > 0 for an incomplete one (unused bit patterns decode as "no code"); *n_codes = symbols with a code,
// *n_len1 = those of length 1 (zlib lets an incomplete code pass only when n_codes == n_len1).  The lanes take a code length each.
template <class W, int PB, int NSYM>
ED_INF_HD int huff_build(W& w, Huff<PB, NSYM>& h, const uint8_t* lens, int n, int* n_codes, int* n_len1)
{
  w.sync();                                                   // lens is complete; nobody decodes with the previous tables any more
  for (int i = w.lane(); i < (1 << PB); i += w.lanes()) h.fast[i] = 0;
  for (int l = w.lane(); l < 16; l += w.lanes()) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += lens[i] == l;
    h.count[l] = (uint16_t)c;
  }
  w.sync();
  int left = 1, codes = 0;
  for (int l = 1; l <= 15; ++l) {
    left <<= 1;
    left -= (int)h.count[l];
    codes += (int)h.count[l];
    if (left < 0) return -1;
  }
  *n_codes = codes;
  *n_len1 = (int)h.count[1];
  for (int l = 1 + w.lane(); l <= 15; l += w.lanes()) {
    if (h.count[l] == 0) continue;
    uint32_t code = 0, off = 0;                               // first code of length l, and where its symbols begin
    for (int j = 1; j < l; ++j) { code = (code + h.count[j]) << 1; off += h.count[j]; }
    for (int i = 0; i < n; ++i) {
      if (lens[i] != l) continue;
      h.sym[off++] = (uint16_t)i;
      if (l <= PB) {
        const uint16_t e = (uint16_t)((l << 12) | i);
        for (uint32_t k = bit_reverse(code, l); k < (1u << PB); k += 1u << l) h.fast[k] = e;
      }
      ++code;
    }
  }
  w.sync();
  return left;
}

// The next symbol, or -1 when the next 15 bits (zeros past the end of the data) begin no code.  *max_len keeps the longest code seen.
template <int PB, int NSYM>
ED_INF_HD int huff_decode(const Huff<PB, NSYM>& h, BitReader& br, int* max_len)
{
  uint32_t bits = br.peek(15);
  const uint32_t e = h.fast[bits & ((1u << PB) - 1u)];
  if (e) {
    const int l = (int)(e >> 12);
    if (l > *max_len) *max_len = l;
    br.drop((uint32_t)l);
    return (int)(e & 0xfffu);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int c = (int)h.count[l];
    if (code - c < first) {
      if (l > *max_len) *max_len = l;
      br.drop((uint32_t)l);
      return (int)h.sym[index + (code - first)];
    }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------------- lengths and distances (RFC 1951, 3.2.5)
// The base / extra-bits tables in closed form (tools/inflate_check.cpp compares every entry with the RFC's lists).  Length symbols are given as
// symbol - 257: 0 .. 28; 29 and 30 (symbols 286, 287) and distance symbols 30, 31 have no meaning and are the caller's BAD_SYMBOL.
ED_INF_HD void length_code(uint32_t s, uint32_t* base, uint32_t* extra)
{
  if (s < 8) { *base = 3 + s; *extra = 0; }
  else if (s == 28) { *base = 258; *extra = 0; }
  else { *extra = (s - 4) >> 2; *base = 3 + ((4 + (s & 3u)) << *extra); }
}
ED_INF_HD void distance_code(uint32_t s, uint32_t* base, uint32_t* extra)
{
  if (s < 4) { *base = 1 + s; *extra = 0; }
  else { *extra = (s >> 1) - 1; *base = 1 + ((2 + (s & 1u)) << *extra); }
}
// position of the k-th code-length code length (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15), five bits each
ED_INF_HD uint32_t code_length_order(uint32_t k)
{
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45
                      | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31u);
}

// ---------------------------------------------------------------------------------------------- CRC-32 (zlib's: reflected 0xEDB88320)
constexpr uint32_t kCrcPoly = 0xedb88320u;

ED_INF_HD uint32_t crc32_table_entry(uint32_t i)
{
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
// the CRC-32 of p[0, n) as zlib.crc32 gives it (a slice's own: initial value and final complement included); tab: crc32_table_entry(0 .. 255)
ED_INF_HD uint32_t crc32_bytes(const uint32_t* tab, const uint8_t* p, uint32_t n)
{
  uint32_t c = 0xffffffffu;
  for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return ~c;
}
// a(x) * b(x) mod P(x) in the reflected representation (bit 31 = x^0)
ED_INF_HD uint32_t crc32_mulmod(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// crc of A -> the part it contributes to crc of A || B where B has n_bytes bytes: crc * x^(8 n_bytes) mod P.  With that,
//   crc(A || B) = crc32_shift(crc(A), len(B)) ^ crc(B)
// and, the operator being linear, a stream cut into slices has  crc = XOR over slices of crc32_shift(crc(slice), bytes after the slice).
ED_INF_HD uint32_t crc32_shift(uint32_t crc, uint32_t n_bytes)
{
  uint32_t p = 1u << 31;                                      // 1
  uint32_t sq = 1u << 23;                                     // x^8
  for (uint32_t n = n_bytes; n; n >>= 1) {
    if (n & 1u) p = crc32_mulmod(sq, p);
    sq = crc32_mulmod(sq, sq);
  }
  return crc32_mulmod(p, crc);
}

// ---------------------------------------------------------------------------------------------- the decoder
struct Tables {                 // an executor's working set: about 3.9 KiB (LDS on the device)
  Huff<10, 288> lit;
  Huff<8, 32> dist;
  Huff<7, 19> cl;
  uint8_t lens[288 + 32];
  uint8_t cl_lens[19];
};

struct Report { int32_t max_code_len; int32_t n_deflate_blocks; };

// One thread.  out has room for exactly cap bytes.
struct Serial {
  uint8_t* out;
  uint32_t pos, cap;            // bytes put so far; ISIZE
  const uint32_t* crc_tab;
  ED_INF_HD int lane() const { return 0; }
  ED_INF_HD int lanes() const { return 1; }
  ED_INF_HD void sync() {}
  ED_INF_HD void flush() {}
  ED_INF_HD bool literal(uint32_t b) { if (pos >= cap) return false; out[pos++] = (uint8_t)b; return true; }
  ED_INF_HD uint32_t xor_all(uint32_t v) const { return v; }
};

// P::kLanes lanes, one value of this type a lane.  Literals are collected a lane each (lane k holds the k-th pending one) and stored kLanes at a
// time, or when a copy needs them in place (flush).  pos counts the pending literals too; np and mine are the same in every lane at every step,
// so no lane waits for another here.  The primitive P supplies what the machine has: kLanes, sync() -- a barrier of the lanes after which each
// sees what the others wrote before it -- and xor_all(v), the XOR of every lane's v, called by all lanes.  The kernel's is in edinflate.inc
// (a wavefront); tools/inflate_lanes_check.cpp runs this text on emulated lanes under adversarial schedules.
template <class P>
struct Lanes {
  uint8_t* out;
  uint32_t pos, cap;
  const uint32_t* crc_tab;
  int ln;
  uint32_t np, mine;           // literals collected and not stored yet; this lane's
  P prim;
  ED_INF_HD int lane() const { return ln; }
  ED_INF_HD int lanes() const { return P::kLanes; }
  ED_INF_HD void sync() { prim.sync(); }
  ED_INF_HD void flush() { if ((uint32_t)ln < np) out[pos - np + (uint32_t)ln] = (uint8_t)mine; np = 0; }
  ED_INF_HD bool literal(uint32_t b)
  {
    if (pos >= cap) return false;
    if ((uint32_t)ln == np) mine = b;
    ++np; ++pos;
    if (np == (uint32_t)P::kLanes) flush();
    return true;
  }
  ED_INF_HD uint32_t xor_all(uint32_t v) { return prim.xor_all(v); }
};

// len bytes from `dist` back.  With dist < len the source is periodic, so every byte is read from what lay there before the copy began.
template <class W>
ED_INF_HD void copy_match(W& w, uint32_t len, uint32_t dist)
{
  w.flush();
  w.sync();
  uint8_t* o = w.out + w.pos;
  const uint8_t* s = o - dist;
  if (dist >= len) for (uint32_t i = (uint32_t)w.lane(); i < len; i += (uint32_t)w.lanes()) o[i] = s[i];
  else for (uint32_t i = (uint32_t)w.lane(); i < len; i += (uint32_t)w.lanes()) o[i] = s[i % dist];
  w.pos += len;
}

template <class W>
ED_INF_HD int inflate_codes(W& w, Tables& t, BitReader& br, Report& rep)
{
  for (;;) {
    int s = huff_decode(t.lit, br, &rep.max_code_len);
    if (br.over) return INPUT_OVERRUN;
    if (s < 0) return br.avail() < 15 ? INPUT_OVERRUN : BAD_SYMBOL;
    if (s < 256) {
      if (!w.literal((uint32_t)s)) return OUTPUT_OVERRUN;
      continue;
    }
    if (s == 256) return OK;
    s -= 257;
    if (s >= 29) return BAD_SYMBOL;
    uint32_t base, extra;
    length_code((uint32_t)s, &base, &extra);
    const uint32_t len = base + br.get(extra);
    const int d = huff_decode(t.dist, br, &rep.max_code_len);
    if (br.over) return INPUT_OVERRUN;
    if (d < 0) return br.avail() < 15 ? INPUT_OVERRUN : BAD_SYMBOL;
    if (d >= 30) return BAD_SYMBOL;
    distance_code((uint32_t)d, &base, &extra);
    const uint32_t dist = base + br.get(extra);
    if (br.over) return INPUT_OVERRUN;
    if (dist > w.pos) return BAD_DISTANCE;
    if (len > w.cap - w.pos) return OUTPUT_OVERRUN;
    copy_match(w, len, dist);
  }
}

template <class W>
ED_INF_HD int read_dynamic_tables(W& w, Tables& t, BitReader& br, Report& rep)
{
  const uint32_t nlen = br.get(5) + 257, ndist = br.get(5) + 1, ncode = br.get(4) + 4;
  if (br.over) return INPUT_OVERRUN;
  if (nlen > 286 || ndist > 30) return BAD_CODE_LENGTHS;
  w.sync();
  for (uint32_t i = 0; i < 19; ++i) t.cl_lens[i] = 0;
  for (uint32_t i = 0; i < ncode; ++i) t.cl_lens[code_length_order(i)] = (uint8_t)br.get(3);
  if (br.over) return INPUT_OVERRUN;
  int n_codes = 0, n_len1 = 0;
  if (huff_build(w, t.cl, t.cl_lens, 19, &n_codes, &n_len1) != 0) return BAD_CODE_LENGTHS;       // zlib wants this one complete
  const uint32_t total = nlen + ndist;
  for (uint32_t i = 0; i < total;) {
    const int s = huff_decode(t.cl, br, &rep.max_code_len);
    if (br.over) return INPUT_OVERRUN;
    if (s < 0) return br.avail() < 15 ? INPUT_OVERRUN : BAD_CODE_LENGTHS;
    if (s < 16) { t.lens[i++] = (uint8_t)s; continue; }
    uint32_t prev = 0, n;
    if (s == 16) {
      if (i == 0) return BAD_CODE_LENGTHS;
      prev = t.lens[i - 1];
      n = 3 + br.get(2);
    } else if (s == 17) n = 3 + br.get(3);
    else n = 11 + br.get(7);
    if (br.over) return INPUT_OVERRUN;
    if (i + n > total) return BAD_CODE_LENGTHS;
    while (n--) t.lens[i++] = (uint8_t)prev;
  }
  if (t.lens[256] == 0) return BAD_CODE_LENGTHS;
  int left = huff_build(w, t.lit, t.lens, (int)nlen, &n_codes, &n_len1);
  if (left < 0 || (left > 0 && n_codes != n_len1)) return BAD_CODE_LENGTHS;
  left = huff_build(w, t.dist, t.lens + nlen, (int)ndist, &n_codes, &n_len1);
  if (left < 0 || (left > 0 && n_codes != n_len1)) return BAD_CODE_LENGTHS;
  return OK;
}

template <class W>
ED_INF_HD void fixed_tables(W& w, Tables& t)
{
  w.sync();
  for (int i = w.lane(); i < 288; i += w.lanes()) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = w.lane(); i < 32; i += w.lanes()) t.lens[288 + i] = 5;
  int a, b;
  (void)huff_build(w, t.lit, t.lens, 288, &a, &b);
  (void)huff_build(w, t.dist, t.lens + 288, 32, &a, &b);
}

// The DEFLATE stream of data[0, n) into w.out[0, w.cap), then the length and the CRC-32 against the trailer's.
template <class W>
ED_INF_HD int inflate_stream(W& w, Tables& t, const uint8_t* data, uint32_t n, uint32_t crc, Report& rep)
{
  BitReader br;
  br.init(data, n);
  for (;;) {
    const uint32_t last = br.get(1), type = br.get(2);
    if (br.over) return INPUT_OVERRUN;
    ++rep.n_deflate_blocks;
    int st = OK;
    if (type == 0) {
      br.align();
      const uint32_t len = br.get(16), nlen = br.get(16);
      if (br.over) return INPUT_OVERRUN;
      if (len != (nlen ^ 0xffffu)) return BAD_STORED_LEN;
      const uint32_t at = br.byte_pos();
      if (len > n - at) return INPUT_OVERRUN;
      w.flush();
      if (len > w.cap - w.pos) return OUTPUT_OVERRUN;
      for (uint32_t i = (uint32_t)w.lane(); i < len; i += (uint32_t)w.lanes()) w.out[w.pos + i] = data[at + i];
      w.pos += len;
      br.seek(at + len);
    } else if (type == 1) {
      fixed_tables(w, t);
      st = inflate_codes(w, t, br, rep);
    } else if (type == 2) {
      st = read_dynamic_tables(w, t, br, rep);
      if (st == OK) st = inflate_codes(w, t, br, rep);
    } else return BAD_BTYPE;
    if (st != OK) return st;
    if (last) break;
  }
  w.flush();
  if (w.pos != w.cap) return SIZE_MISMATCH;
  w.sync();
  const uint32_t slice = (w.cap + (uint32_t)w.lanes() - 1) / (uint32_t)w.lanes();
  const uint32_t a = (uint32_t)w.lane() * slice < w.cap ? (uint32_t)w.lane() * slice : w.cap;
  const uint32_t b = a + slice < w.cap ? a + slice : w.cap;
  const uint32_t c = w.xor_all(crc32_shift(crc32_bytes(w.crc_tab, w.out + a, b - a), w.cap - b));
  return c == crc ? OK : BAD_CRC;
}

// The plain serial form: one whole BGZF block of `size` bytes into out, which has room for exactly `isize` bytes -- the block's own ISIZE, which the
// caller has read with block_info.  crc_tab: crc32_table_entry(0 .. 255).  rep may be NULL.
inline int inflate_block(const uint8_t* block, uint32_t size, uint8_t* out, uint32_t isize, const uint32_t* crc_tab, Tables* tables, Report* rep)
{
  BlockInfo bi;
  if (int st = block_info(block, size, &bi)) return st;
  if (bi.isize != isize) return SIZE_MISMATCH;
  Serial w{out, 0, isize, crc_tab};
  Report r{0, 0};
  const int st = inflate_stream(w, *tables, block + bi.data_off, bi.data_len, bi.crc, r);
  if (rep) *rep = r;
  return st;
}

}  // namespace edinf
