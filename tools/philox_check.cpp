// philox_check.cpp -- the uniform of csrc/ed_philox.hpp as a stand-alone host program, to be run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o philox_check tools/philox_check.cpp && ./philox_check
//
// It includes only that header and asserts
//   the three known answers of Philox4x32-10 (counter 0 / key 0, all ones, the digits of pi);
//   the mapping of the 52 bits to a double at k = 0 (2^-53) and k = 2^52 - 1 (1 - 2^-53), and that it is exact for bits around both;
//   the header's loop against a second, straight-line statement of the ten rounds on a few thousand counters, exons >= 2^31 and seeds
//   above 2^32 among them, and the key / counter layout of u53.
// `philox_check --emit` instead reads lines "seed exon sample replicate stream" (decimal, unsigned) from standard input and prints, per
// line, the four output words and the uniform's bit pattern in hex: what tests/test_simulate_host.py compares with its Python restatement.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../exomedepth_amd/csrc/ed_philox.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

// one round written out, no loop and no shared helper
void round_once(uint32_t c[4], uint32_t k[2])
{
  const uint64_t a = 0xD2511F53ull * (uint64_t)c[0];
  const uint64_t b = 0xCD9E8D57ull * (uint64_t)c[2];
  const uint32_t hi_a = (uint32_t)(a >> 32), lo_a = (uint32_t)(a & 0xffffffffull);
  const uint32_t hi_b = (uint32_t)(b >> 32), lo_b = (uint32_t)(b & 0xffffffffull);
  const uint32_t o0 = hi_b ^ c[1] ^ k[0], o1 = lo_b, o2 = hi_a ^ c[3] ^ k[1], o3 = lo_a;
  c[0] = o0; c[1] = o1; c[2] = o2; c[3] = o3;
}
void bump(uint32_t k[2]) { k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u; }

void straight(uint32_t c[4], uint32_t k[2])
{
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k); bump(k);
  round_once(c, k);
}

void known(const uint32_t c[4], const uint32_t k[2], const uint32_t want[4])
{
  const edphilox::Words o = edphilox::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
  for (int i = 0; i < 4; ++i) CHECK(o.w[i] == want[i]);
}

uint64_t bits_of(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s; }

int emit()
{
  unsigned long long seed, e, s, r, st;
  while (std::scanf("%llu %llu %llu %llu %llu", &seed, &e, &s, &r, &st) == 5) {
    const edphilox::Words o =
        edphilox::philox4x32_10((uint32_t)e, (uint32_t)s, (uint32_t)r, (uint32_t)st, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    const double u = edphilox::u53((uint64_t)seed, (uint32_t)e, (uint32_t)s, (uint32_t)r, (uint32_t)st);
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %016" PRIx64 "\n", o.w[0], o.w[1], o.w[2], o.w[3], bits_of(u));
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc > 1 && std::strcmp(argv[1], "--emit") == 0) return emit();
  {
    const uint32_t c[4] = {0, 0, 0, 0}, k[2] = {0, 0}, w[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    known(c, k, w);
  }
  {
    const uint32_t c[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, k[2] = {0xffffffffu, 0xffffffffu};
    const uint32_t w[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
    known(c, k, w);
  }
  {
    const uint32_t c[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k[2] = {0xa4093822u, 0x299f31d0u};
    const uint32_t w[4] = {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    known(c, k, w);
  }
  // the uniform's edges: exact, inside (0, 1)
  CHECK(edphilox::u53_of(0) == 0x1p-53);
  CHECK(edphilox::u53_of((1ull << 52) - 1) == 1.0 - 0x1p-53);
  CHECK(edphilox::u53_of(0) > 0.0 && edphilox::u53_of((1ull << 52) - 1) < 1.0);
  for (uint64_t k = 0; k < 64; ++k) {
    const uint64_t ks[3] = {k, (1ull << 52) - 1 - k, (1ull << 51) + k};
    for (uint64_t v : ks) {
      const double u = edphilox::u53_of(v);
      CHECK(u * 0x1p53 == (double)(2 * v + 1));                      // no bit lost
      CHECK((uint64_t)(u * 0x1p53) == 2 * v + 1);
    }
  }
  // the loop against the straight-line rounds; u53's key and counter layout
  uint64_t st = 0x853c49e6748fea9bull;
  for (int i = 0; i < 6000; ++i) {
    uint32_t c[4], k[2];
    for (int j = 0; j < 4; ++j) c[j] = (uint32_t)(lcg(st) >> 32);
    for (int j = 0; j < 2; ++j) k[j] = (uint32_t)(lcg(st) >> 32);
    if (i % 3 == 0) c[0] |= 0x80000000u;                             // an exon index at or above 2^31, as unsigned
    if (i % 5 == 0) { c[1] = (uint32_t)i; c[2] = (uint32_t)(i % 7); c[3] = (uint32_t)(i & 1); }
    if (i % 11 == 0) k[1] = 0;                                       // a seed below 2^32
    const edphilox::Words o = edphilox::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    uint32_t d[4] = {c[0], c[1], c[2], c[3]}, kk[2] = {k[0], k[1]};
    straight(d, kk);
    for (int j = 0; j < 4; ++j) CHECK(o.w[j] == d[j]);
    const uint64_t seed = ((uint64_t)k[1] << 32) | k[0];
    const double u = edphilox::u53(seed, c[0], c[1], c[2], c[3]);
    const uint64_t kbits = ((uint64_t)(d[0] >> 12) << 32) | d[1];
    CHECK(u == (double)(2 * kbits + 1) * 0x1p-53);
    CHECK(u >= 0x1p-53 && u <= 1.0 - 0x1p-53);
  }
  std::printf("philox_check: %ld checks passed\n", n_checks);
  return 0;
}
