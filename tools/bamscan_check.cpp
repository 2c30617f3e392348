// bamscan_check.cpp -- the BAM record scanner (csrc/ed_bamscan.hpp, the body of ed_bam_scan_records) as a stand-alone program, to be run under
// the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bamscan_check tools/bamscan_check.cpp && ./bamscan_check
//
// Every buffer handed to the scanner is a heap block of EXACTLY n_bytes (so a read one byte past it is an AddressSanitizer report), and the output
// arrays hold exactly `cap` entries.  It runs the scanner over a valid stream, over every truncation of it, over every single-byte corruption of
// every block_size word (all 255 other values of each of its four bytes), and with every cap from 0 up; what it checks besides the sanitizers'
// silence: the records before the stopping point are right, bytes_consumed is a record boundary, and a bad block_size is reported where it lies.
// Exit status 0 and a line of totals on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../exomedepth_amd/csrc/ed_bamscan.hpp"

namespace {

struct Rec { int32_t refid, pos, tlen; uint32_t flag_mapq; int64_t offset; int32_t block_size; };

void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
void put16(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 2; ++k) b.push_back((uint8_t)(v >> (8 * k))); }

uint32_t rng_state = 12345u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

std::vector<uint8_t> make_stream(int n, std::vector<Rec>& recs)
{
  std::vector<uint8_t> b;
  for (int i = 0; i < n; ++i) {
    const int32_t extra = (int32_t)(i == 0 ? 0 : rnd() % 90);          // the first record has nothing after its fixed part: block_size == 32
    Rec r{(int32_t)(rnd() % 5) - 1, (int32_t)(rnd() % 100000), (int32_t)(rnd() % 2001) - 1000, 0u, (int64_t)b.size(), 32 + extra};
    const uint32_t flag = rnd() % 4096, mapq = rnd() % 256;
    r.flag_mapq = flag | (mapq << 16);
    put32(b, (uint32_t)r.block_size);
    put32(b, (uint32_t)r.refid); put32(b, (uint32_t)r.pos);
    b.push_back((uint8_t)1); b.push_back((uint8_t)mapq); put16(b, 4680); put16(b, 0); put16(b, flag);
    put32(b, 0); put32(b, 0xffffffffu); put32(b, 0xffffffffu); put32(b, (uint32_t)r.tlen);
    for (int k = 0; k < extra; ++k) b.push_back((uint8_t)rnd());
    recs.push_back(r);
  }
  return b;
}

int fail(const char* what, long long a, long long b)
{
  std::fprintf(stderr, "bamscan_check: FAILED: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

// one scan of the first n bytes of `stream` in an exact-size heap block, with exact-size outputs; *n_out / *used_out / *rc_out describe it
int scan_exact(const std::vector<uint8_t>& stream, int64_t n, int64_t cap, const std::vector<Rec>& recs, int64_t* n_out, int64_t* used_out,
               int* rc_out, int64_t* bad_off, int32_t* bad_val)
{
  uint8_t* buf = (uint8_t*)std::malloc((size_t)(n ? n : 1));
  if (n) std::memcpy(buf, stream.data(), (size_t)n);
  int32_t* refid = (int32_t*)std::malloc((size_t)(cap ? cap : 1) * 4);
  int32_t* pos = (int32_t*)std::malloc((size_t)(cap ? cap : 1) * 4);
  int32_t* tlen = (int32_t*)std::malloc((size_t)(cap ? cap : 1) * 4);
  uint32_t* fm = (uint32_t*)std::malloc((size_t)(cap ? cap : 1) * 4);
  *rc_out = edbam::scan_records(n ? buf : nullptr, n, cap, refid, pos, tlen, fm, n_out, used_out, bad_off, bad_val);
  int bad = 0;
  if (*n_out < 0 || *n_out > cap || *n_out > (int64_t)recs.size()) bad = fail("record count out of range", *n_out, cap);
  for (int64_t i = 0; !bad && i < *n_out; ++i)
    if (refid[i] != recs[(size_t)i].refid || pos[i] != recs[(size_t)i].pos || tlen[i] != recs[(size_t)i].tlen || fm[i] != recs[(size_t)i].flag_mapq)
      bad = fail("record fields differ", i, n);
  if (!bad) {
    const int64_t want = *n_out < (int64_t)recs.size() ? recs[(size_t)*n_out].offset : (int64_t)stream.size();
    if (*used_out != want) bad = fail("bytes_consumed is not the boundary after the last record read", *used_out, want);
    if (*used_out > n) bad = fail("bytes_consumed beyond the buffer", *used_out, n);
  }
  std::free(buf); std::free(refid); std::free(pos); std::free(tlen); std::free(fm);
  return bad;
}

}  // namespace

int main()
{
  std::vector<Rec> recs;
  const std::vector<uint8_t> stream = make_stream(40, recs);
  const int64_t N = (int64_t)stream.size(), R = (int64_t)recs.size();
  int64_t n = 0, used = 0, bad_off = 0, n_scans = 0, n_rejected = 0;
  int32_t bad_val = 0;
  int rc = 0;
  // the valid stream, every cap
  for (int64_t cap = 0; cap <= R + 2; ++cap) {
    if (scan_exact(stream, N, cap, recs, &n, &used, &rc, &bad_off, &bad_val)) return 1;
    if (rc != edbam::kScanOk || n != (cap < R ? cap : R)) return fail("valid stream", n, cap);
    ++n_scans;
  }
  // every truncation: the records wholly inside are read, the cut one is left, no error
  for (int64_t cut = 0; cut <= N; ++cut) {
    if (scan_exact(stream, cut, R + 1, recs, &n, &used, &rc, &bad_off, &bad_val)) return 1;
    int64_t whole = 0;
    while (whole < R && recs[(size_t)whole].offset + 4 + recs[(size_t)whole].block_size <= cut) ++whole;
    if (rc != edbam::kScanOk || n != whole) return fail("truncation", cut, n);
    ++n_scans;
  }
  // every single-byte corruption of every block_size word, whole stream and cut in the middle of the corrupted record
  for (int64_t i = 0; i < R; ++i)
    for (int byte = 0; byte < 4; ++byte)
      for (int v = 0; v < 256; ++v) {
        std::vector<uint8_t> s = stream;
        uint8_t& b = s[(size_t)recs[(size_t)i].offset + (size_t)byte];
        if (b == (uint8_t)v) continue;
        b = (uint8_t)v;
        const int32_t bs = (int32_t)edbam::le32(&s[(size_t)recs[(size_t)i].offset]);
        for (int64_t cut : {N, recs[(size_t)i].offset + 4 + 16, recs[(size_t)i].offset + 3}) {
          if (cut > N) cut = N;
          uint8_t* buf = (uint8_t*)std::malloc((size_t)cut);
          std::memcpy(buf, s.data(), (size_t)cut);
          std::vector<int32_t> a((size_t)R + 1), p((size_t)R + 1), t((size_t)R + 1);
          std::vector<uint32_t> f((size_t)R + 1);
          rc = edbam::scan_records(buf, cut, R + 1, a.data(), p.data(), t.data(), f.data(), &n, &used, &bad_off, &bad_val);
          std::free(buf);
          ++n_scans;
          const bool word_inside = recs[(size_t)i].offset + 4 <= cut;
          const bool invalid = bs < edbam::kFixed || bs > edbam::kMaxBlock;
          if (word_inside && invalid) {
            if (rc != edbam::kScanBadBlock || bad_off != recs[(size_t)i].offset || bad_val != bs || n != i || used != recs[(size_t)i].offset)
              return fail("a bad block_size was not reported where it lies", i, bs);
            ++n_rejected;
          } else {
            // a valid other size sends the chain somewhere else: whatever is read from there on must stay inside the buffer (the sanitizer
            // watches that), bytes_consumed inside it, and the records before the changed word as they were
            if (n < (word_inside ? 0 : i) || used > cut || used < 0) return fail("scan left the buffer after a changed block_size", i, used);
            for (int64_t k = 0; k < i && k < n; ++k)
              if (a[(size_t)k] != recs[(size_t)k].refid || t[(size_t)k] != recs[(size_t)k].tlen) return fail("records before the corruption differ", i, k);
          }
        }
      }
  std::printf("bamscan_check ok: %lld records, %lld bytes, %lld scans, %lld bad block_size words reported, none read outside its buffer\n",
              (long long)R, (long long)N, (long long)n_scans, (long long)n_rejected);
  return 0;
}
