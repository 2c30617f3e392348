// ed_philox.hpp -- the uniform behind every draw from the fitted model (csrc/edsim.inc), written once for the host and for the
// device.  No HIP include and nothing of the library's: gcc compiles it as it is (tools/philox_check.cpp runs it under the host sanitizers),
// hipcc compiles the same text for gfx950.
//
// Generator.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) from its published
// definition: a round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
//   (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))          M0 = 0xD2511F53, M1 = 0xCD9E8D57
// with hi / lo the halves of the 64-bit product, and the key goes up by (0x9E3779B9, 0xBB67AE85) between rounds; ten rounds.
// Key and counter (a contract): key = (seed & 0xffffffff, seed >> 32) of a 64-bit seed; counter = (exon, sample,
// replicate, stream): the exon's index in the plan, the GLOBAL sample index, the replicate, and 0 for the null draw / 1 for planted cells.
// The uniform.  From the output words w0 .. w3: k = (w0 >> 12) 2^32 + w1 (52 bits), u = (2 k + 1) 2^-53: exact in binary64,
// 2^-53 <= u <= 1 - 2^-53, never 0 and never 1.  w2 and w3 are unused and reserved.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ED_PHILOX_HD __host__ __device__ inline
#else
#define ED_PHILOX_HD inline
#endif

namespace edphilox {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;
constexpr int kRounds = 10;
constexpr uint32_t kStreamNull = 0, kStreamPlanted = 1;

struct Words { uint32_t w[4]; };

ED_PHILOX_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t p0 = (uint64_t)kMul0 * c0, p1 = (uint64_t)kMul1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += kKey0; k1 += kKey1;
  }
  return Words{{c0, c1, c2, c3}};
}

// the 52 bits of a uniform to the double: (2 k + 1) 2^-53, k < 2^52 (2 k + 1 < 2^53 is a whole double; the scaling is a power of two)
ED_PHILOX_HD double u53_of(uint64_t k) { return (double)(2 * k + 1) * 0x1p-53; }

ED_PHILOX_HD double u53(uint64_t seed, uint32_t exon, uint32_t sample, uint32_t replicate, uint32_t stream)
{
  const Words o = philox4x32_10(exon, sample, replicate, stream, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  return u53_of(((uint64_t)(o.w[0] >> 12) << 32) | o.w[1]);
}

}  // namespace edphilox
