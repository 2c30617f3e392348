// ed_mix_plan.hpp -- launch geometry of the mixture profile (csrc/edmix.inc: k_mix_profile).  Host-only: no HIP, no
// device types; tools/mix_plan_check.cpp checks it stand-alone.  The kernel reads the constants and the constexpr functions.
//
// A workgroup of kThreads = 4 waves serves ONE chain -- one (pair, chromosome) -- at all the pair's grid points:
//   wave 0          walks the chain: 16 quads of lanes, quad q at grid point quad_grid(q, G); quads q >= G shadow the last grid point and
//                   store nothing
//   waves 1 .. 3    evaluate the emissions of the NEXT tile of kTile exons into LDS, one column a wave and pass, one exon a lane:
//                   column 0 is the normal state (it does not depend on the mixture), column 1 + 2 g the deletion and 2 + 2 g the
//                   duplication state at grid point g -- n_cols(G) = 1 + 2 G columns, a row of kRowStride doubles per exon
// Two tiles (the one walked, the one filled), per exon its row of emissions and the three log-transitions (A, B, C and a pad) of its gap.
// The launch grid is (pairs, jobs): job y is chromosome job_chrom[y] of job_order() -- the non-empty chromosomes, longest first, ties in
// index order -- so the longest chains start first.  An empty chromosome is in no job: its log-evidence stays at the 0 the host wrote.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace edmix {

constexpr int kTile = 64;                    // exons per tile
constexpr int kMaxGrid = 16;                 // grid points per launch: the quads of the chain wave
constexpr int kPairsPerWg = 1;
constexpr int kThreads = 256;
constexpr int kEmitWaves = kThreads / 64 - 1;
constexpr int kRowStride = 1 + 2 * kMaxGrid; // doubles per exon in a tile (odd: the lanes of a pass write 64 different banks)
constexpr int kLtStride = 4;                 // doubles per exon of log-transitions: A, B, C, pad
constexpr int kLogTableBytes = 3 * 1024;     // room for ed_plog's table (edpost.inc: lse3), checked against its size where it is parked
constexpr int kLdsLimit = 64 * 1024;         // static shared memory of a workgroup

constexpr int n_cols(int G) { return 1 + 2 * G; }
constexpr int col_del(int g) { return 1 + 2 * g; }
constexpr int col_dup(int g) { return 2 + 2 * g; }
// the grid point of quad q of the chain wave, and whether the quad stores
constexpr int quad_grid(int q, int G) { return q < G ? q : G - 1; }
constexpr bool quad_live(int q, int G) { return q < G; }

constexpr int n_tiles(int m) { return (m + kTile - 1) / kTile; }
constexpr int tile_first(int t) { return t * kTile; }
constexpr int tile_count(int m, int t) { return m - t * kTile < kTile ? m - t * kTile : kTile; }

// bytes of LDS of a workgroup: two tiles of emissions and log-transitions, the constants of the columns (a1, a2, log B(a1, a2)), ed_plog's table
constexpr int lds_bytes()
{
  return 2 * kTile * (kRowStride + kLtStride) * 8 + 3 * kRowStride * 8 + kLogTableBytes;
}

// the non-empty chromosomes, longest first, ties in index order: out[y] is the chromosome of launch row y
inline std::vector<int32_t> job_order(int32_t C, const int32_t* chrom_off)
{
  std::vector<int32_t> out;
  for (int32_t c = 0; c < C; ++c)
    if (chrom_off[c + 1] - chrom_off[c] > 0) out.push_back(c);
  std::stable_sort(out.begin(), out.end(), [&](int32_t a, int32_t b) {
    return chrom_off[a + 1] - chrom_off[a] > chrom_off[b + 1] - chrom_off[b];
  });
  return out;
}

// what workgroup (x, y) of the launch serves
struct Job {
  int64_t pair;
  int32_t chrom;
};
inline Job job_of(int64_t block_x, int32_t block_y, const std::vector<int32_t>& job_chrom) { return Job{block_x, job_chrom[(size_t)block_y]}; }

}  // namespace edmix
