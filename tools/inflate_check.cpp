// inflate_check.cpp -- the BGZF block decoder (csrc/ed_inflate.hpp: the serial inflate_block, the same rules k_bgzf_inflate runs on the device)
// as a stand-alone program without zlib, to be run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o inflate_check tools/inflate_check.cpp && ./inflate_check CASES [--sample]
//
// CASES is written by tests/test_inflate_host.py (Python's zlib is the other side): "EDINFCS1", uint32 n, then per case
//   uint32 block bytes, uint32 0 = must be refused / 1 = must be accepted / 2 = accepted, and its truncations are run, uint32 expected bytes, the block, the expected bytes
// all little-endian.  Every block is handed to inflate_block in a heap block of EXACTLY its length and the output in one of ISIZE bytes (of
// min(ISIZE, 2064 n + 1) where a corrupted trailer names more than n input bytes can give: see run()), so a byte read or written outside either is
// an AddressSanitizer report.  Checked: a case that must be accepted gives OK and the expected bytes; one
// that must be refused gives a status other than OK.  For every accepted case (1 or 2) EVERY truncation of the block is run too.  With --sample (the
// pytest run, which has to stay quick: the full set is quadratic in a block's length, 2 * 10^9 byte steps for one stored block of 65 290) only the
// cases marked 2 are truncated, and of a block above 4096 bytes only within 600 bytes of either end and every 251st between; the totals line
// says how many truncations the sampling left out.  A truncation may come out as anything but a fault.  Also checked here, without a case file: the
// closed forms of the length / distance tables against RFC 1951's lists, the code-length order, and the CRC-32 slice-and-shift identity.
// One line per case on stdout ("case K status NAME max_code_len L deflate_blocks B"), then a line of totals starting with "ok"; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(__GLIBC__)
#include <malloc.h>
#endif

#include "../exomedepth_amd/csrc/ed_inflate.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

uint32_t crc_tab[256];

// the block in a heap block of exactly n bytes, the output in one of ISIZE (bounded as below); returns the status (and the output, when out is given)
int run(const uint8_t* block, uint32_t n, std::vector<uint8_t>* out, edinf::Report* rep)
{
  uint8_t* b = (uint8_t*)std::malloc(n ? n : 1);
  std::memcpy(b, block, n);
  edinf::BlockInfo bi{};
  int st = edinf::block_info(b, n, &bi);
  if (st == edinf::OK) {
    // exactly ISIZE bytes -- unless the trailer names more than n bytes of DEFLATE data can give at all (a match of 258 bytes takes two bits at
    // least: under 2064 bytes per input byte), as a corrupted ISIZE of gigabytes does: then that bound, which the decoder cannot reach either
    const size_t most = (size_t)2064 * n + 1, room = bi.isize < most ? bi.isize : most;
    uint8_t* o = (uint8_t*)std::malloc(room ? room : 1);
    edinf::Tables* t = (edinf::Tables*)std::malloc(sizeof(edinf::Tables));
    st = edinf::inflate_block(b, n, o, bi.isize, crc_tab, t, rep);
    if (out && st == edinf::OK) out->assign(o, o + bi.isize);
    std::free(t);
    std::free(o);
  }
  std::free(b);
  return st;
}

void check_tables()
{
  static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                8193, 12289, 16385, 24577};
  static const int dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (uint32_t s = 0; s < 29; ++s) {
    uint32_t b, e;
    edinf::length_code(s, &b, &e);
    CHECK((int)b == lbase[s] && (int)e == lext[s], "length symbol %u: base %u extra %u", 257 + s, b, e);
  }
  for (uint32_t s = 0; s < 30; ++s) {
    uint32_t b, e;
    edinf::distance_code(s, &b, &e);
    CHECK((int)b == dbase[s] && (int)e == dext[s], "distance symbol %u: base %u extra %u", s, b, e);
  }
  for (uint32_t k = 0; k < 19; ++k) CHECK((int)edinf::code_length_order(k) == order[k], "code-length order %u", k);
}

void check_crc()
{
  const char* s = "123456789";
  CHECK(edinf::crc32_bytes(crc_tab, (const uint8_t*)s, 9) == 0xcbf43926u, "crc32 of the check string");
  std::vector<uint8_t> v(5000);
  uint32_t x = 99u;
  for (auto& b : v) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
  for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 1000u, 5000u}) {
    const uint32_t whole = edinf::crc32_bytes(crc_tab, v.data(), n);
    for (uint32_t lanes : {1u, 3u, 64u}) {
      const uint32_t slice = (n + lanes - 1) / lanes;
      uint32_t c = 0;
      for (uint32_t l = 0; l < lanes; ++l) {
        const uint32_t a = l * slice < n ? l * slice : n, b = a + slice < n ? a + slice : n;
        c ^= edinf::crc32_shift(edinf::crc32_bytes(crc_tab, v.data() + a, b - a), n - b);
      }
      CHECK(c == whole, "crc32 of %u bytes in %u slices", n, lanes);
    }
  }
}

uint32_t rd32(const std::vector<uint8_t>& f, size_t& p) { const uint32_t v = edinf::le32(f.data() + p); p += 4; return v; }

}  // namespace

int main(int argc, char** argv)
{
#if defined(__GLIBC__)
  mallopt(M_TRIM_THRESHOLD, 64 << 20);      // every run allocates and frees its buffers: keep the heap's pages instead of returning them each time
  mallopt(M_MMAP_THRESHOLD, 64 << 20);
#endif
  for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = edinf::crc32_table_entry(i);
  check_tables();
  check_crc();
  long n_cases = 0, n_accepted = 0, n_trunc = 0, n_trunc_ok = 0, n_trunc_skipped = 0;
  const bool sample = argc > 2 && std::strcmp(argv[2], "--sample") == 0;
  if (argc > 1) {
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> f;
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + k);
    std::fclose(fp);
    if (f.size() < 12 || std::memcmp(f.data(), "EDINFCS1", 8) != 0) { std::printf("not a case file\n"); return 2; }
    size_t p = 8;
    const uint32_t n = rd32(f, p);
    for (uint32_t c = 0; c < n; ++c) {
      if (p + 12 > f.size()) { std::printf("case file cut short\n"); return 2; }
      const uint32_t size = rd32(f, p), accept = rd32(f, p), n_exp = rd32(f, p);
      if (p + size + n_exp > f.size()) { std::printf("case file cut short\n"); return 2; }
      const uint8_t* block = f.data() + p;
      const uint8_t* exp = block + size;
      p += (size_t)size + n_exp;
      std::vector<uint8_t> out;
      edinf::Report rep{0, 0};
      const int st = run(block, size, &out, &rep);
      std::printf("case %u status %s max_code_len %d deflate_blocks %d\n", c, edinf::status_name(st), rep.max_code_len, rep.n_deflate_blocks);
      ++n_cases;
      if (accept) {
        ++n_accepted;
        CHECK(st == edinf::OK, "case %u must be accepted: %s", c, edinf::status_name(st));
        CHECK(st != edinf::OK || (out.size() == n_exp && (n_exp == 0 || std::memcmp(out.data(), exp, n_exp) == 0)), "case %u: bytes differ", c);
        for (uint32_t k = 0; k < size; ++k) {
          if (sample && (accept != 2 || (size > 4096 && k > 600 && k + 600 < size && k % 251 != 0))) { ++n_trunc_skipped; continue; }
          ++n_trunc;
          n_trunc_ok += run(block, k, nullptr, nullptr) == edinf::OK;
        }
      } else {
        CHECK(st != edinf::OK, "case %u must be refused", c);
      }
    }
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok: %ld cases (%ld accepted), %ld truncations (%ld left out by --sample, %ld came out OK)\n", n_cases, n_accepted, n_trunc,
              n_trunc_skipped, n_trunc_ok);
  return 0;
}
