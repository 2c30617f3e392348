// ed_power_plan.hpp -- geometry of the detection-power map (csrc/edpower.inc).  Host-only: no HIP, no device types;
// tools/power_plan_check.cpp checks it stand-alone.  The kernels read the constants and the constexpr functions.
//
// Occupancy.  A sample's occupied totals are the set bits of its row of a bit map, bit n of word n / 32.  A total is VALID when
// 0 <= n <= kMaxTotal; an invalid one (above the maximum, or a sum of counts below 0) is skipped: it is in no map, its exons read NaN.
// A row has map_words(largest valid total of the whole map) words: kOccCap / 32 while every valid total is below the occupancy cap
// kOccCap, else kMaxTotal / 32 + 1 -- the wide map is only made where some sample needs it.  The occupied totals of a sample in
// ascending order are its TABLE; slot(n) = the number of set bits below bit n.
// Jobs.  One job per (sample, occupied total).  Job k of a sample is its k-th LARGEST total; the list holds every sample's job 0, then
// every sample's job 1, ... (JobLayout): the longest walks of all samples start first.  Within one k the samples stand in the order of
// their number of jobs, most first, ties in index order, so that the samples that have a job k are the first ns(k) of that order.
// Walk.  One wavefront per job walks x = 0 .. n in tiles of kWalkTile = 64 lanes x kWalkPer values.
// Regions.  One wavefront per (region, sample).  Lane l adds the exons first + l, first + 64 + l, ... of the run in that order, starting
// from +0.0; the 64 lane sums are combined by the tree  p[l] += p[l + d]  (l < d)  for d = 32, 16, 8, 4, 2, 1  (region_sum below is
// that order on the host).
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "ed_rows.hpp"

namespace edpower {

constexpr int kWalkLanes = 64;
constexpr int kWalkPer = 4;                               // values of x per lane and tile
constexpr int kWalkTile = kWalkLanes * kWalkPer;          // 256
constexpr int kWalkWaves = 4;                             // jobs per workgroup
constexpr int32_t kOccCap = 1 << 15;                      // totals below it fit the narrow map
constexpr int32_t kMaxTotal = 1 << 20;                    // the largest total that is walked
constexpr int kRegionTile = 64;                           // exons a wavefront takes per step of a run
constexpr int kRegionWaves = 4;                           // (region, sample) pairs per workgroup
constexpr int kSlotTile = 64;                             // the slot map is written in tiles of 64 exons x 64 samples

static_assert(kOccCap % 32 == 0 && kOccCap < kMaxTotal, "the narrow map is whole words and smaller than the wide one");

constexpr bool total_ok(int64_t n) { return n >= 0 && n <= (int64_t)kMaxTotal; }
constexpr int32_t word_of(int32_t n) { return n >> 5; }
constexpr uint32_t below_mask(int32_t n) { return (1u << (n & 31)) - 1u; }     // the bits of n's word below n's own
constexpr int32_t map_words(int32_t largest) { return largest < kOccCap ? kOccCap / 32 : kMaxTotal / 32 + 1; }
constexpr int64_t n_walk_tiles(int64_t n) { return (n + 1 + kWalkTile - 1) / kWalkTile; }     // x = 0 .. n

// where the jobs of a map stand in its list: job k of sample s (its k-th largest total) is at off_k[k] + rank[s]
struct JobLayout {
  std::vector<int32_t> rank;     // [S]
  std::vector<int64_t> off_k;    // [max jobs of a sample + 1]
  int64_t n_jobs = 0;
  int32_t max_jobs = 0;
};
inline JobLayout job_layout(const int32_t* count, int64_t S)
{
  JobLayout L;
  L.rank.assign((size_t)S, 0);
  std::vector<int64_t> order((size_t)S);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return count[a] > count[b]; });
  for (int64_t i = 0; i < S; ++i) L.rank[(size_t)order[(size_t)i]] = (int32_t)i;
  for (int64_t s = 0; s < S; ++s) L.max_jobs = std::max(L.max_jobs, count[s]);
  // ns(k) = the samples with more than k jobs
  std::vector<int64_t> ns((size_t)L.max_jobs + 1, 0);
  for (int64_t s = 0; s < S; ++s) if (count[s] > 0) ns[(size_t)count[s] - 1] += 1;
  for (int32_t k = L.max_jobs - 1; k >= 0; --k) ns[(size_t)k] += ns[(size_t)k + 1];
  L.off_k.assign((size_t)L.max_jobs + 1, 0);
  for (int32_t k = 0; k < L.max_jobs; ++k) L.off_k[(size_t)k + 1] = L.off_k[(size_t)k] + ns[(size_t)k];
  L.n_jobs = L.off_k[(size_t)L.max_jobs];
  return L;
}

// the sum of a run of n values in the region kernel's order; at(i) is value i of the run
template <class F>
inline double region_sum(int64_t n, F at)
{
  double p[kRegionTile];
  for (int l = 0; l < kRegionTile; ++l) p[l] = 0.0;
  for (int64_t i = 0; i < n; ++i) p[i % kRegionTile] += at(i);
  for (int d = kRegionTile / 2; d >= 1; d >>= 1)
    for (int l = 0; l < d; ++l) p[l] += p[l + d];
  return p[0];
}

using edrows::row_fault;     // a region row against the plan: the region form (ed_rows.hpp)

// the rows of the plan's table a region's price reads, for the run first .. last (exon indices of the plan) of chromosome c: the row of
// the gap in front of exon e is c + e (every chromosome before it has one closing gap more than exons).  N->N and N->T are constants,
// T->T is read from the rows of the inner gaps first + 1 .. last, T->N from the row of the gap behind the run
struct PriceGaps {
  int64_t n_nn;        // gaps charged N->N on the all-normal side: last - first + 2
  int64_t inner0, inner1;   // table rows [inner0, inner1) read for T->T
  int64_t close;       // table row read for T->N
};
constexpr PriceGaps price_gaps(int32_t first, int32_t last, int32_t c)
{
  return PriceGaps{(int64_t)last - first + 2, (int64_t)c + first + 1, (int64_t)c + last + 1, (int64_t)c + last + 1};
}

}  // namespace edpower
