// ed_ratio_plan.hpp -- geometry of the copy-ratio profile (csrc/edratio.inc: k_ratio_profile / k_ratio_sum).  Host-only:
// no HIP, no device types; tools/ratio_plan_check.cpp checks it stand-alone.  The kernels read the constants and the structs.
//
// Rows.  A row is (sample, first exon, last exon), global exon indices, inside one chromosome.
// Items.  A row of n exons is cut from its first exon into segments of at most kSegExons = kSegTiles * kTile exons: segment j holds the
// exons [j * kSegExons, min(n, (j + 1) * kSegExons)) of the row.  One item per (row, segment), rows in index order, a row's segments
// in order; one wavefront serves one item.  Where a segment starts depends on the row's length alone.
// Lanes.  Lane l of an item adds the exons l, l + 64, l + 128, ... of the segment in that order to a double-double that starts at
// (+0, +0); the 64 lane sums are combined by the tree  p[l] += p[l + d]  (l < d)  for d = 32, 16, 8, 4, 2, 1  (segment_sum below is that
// order on the host).
// Rows of one segment are written by their item.  A row of several segments parks its partial sums in a workspace, kMaxGrid slots of
// (hi, lo) per item, and is one entry of the Multi list: k_ratio_sum starts from segment 0's sum and adds the others in index order.
#pragma once

#include <cstdint>
#include <vector>
#include "ed_rows.hpp"

namespace edratio {

constexpr int kTile = 64;                          // exons per tile: a lane each
constexpr int kSegTiles = 8;                       // tiles per segment
constexpr int kSegExons = kSegTiles * kTile;       // 512
constexpr int kNarrow = 0;                         // rows of up to this many exons take the (exon, column) mapping: 0, there is none
constexpr int kMaxGrid = 16;                       // grid points per row and launch
constexpr int kWaves = 4;                          // items per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int64_t kMaxRows = 0x7fffffff;           // a row's index and an item's index are int32 on the device
constexpr int64_t kMaxItems = 0x7fffffff;

constexpr bool grid_ok(int G) { return G >= 1 && G <= kMaxGrid; }
// a dose the model is defined for: -2 < mu <= 2 (a NaN fails both comparisons)
constexpr bool dose_ok(double mu) { return mu > -2.0 && mu <= 2.0; }
constexpr int64_t n_segments(int64_t n) { return (n + kSegExons - 1) / kSegExons; }
constexpr int n_tiles(int count) { return (count + kTile - 1) / kTile; }

struct Item {
  int32_t row;       // index of the row
  int32_t first;     // global index of the segment's first exon
  int32_t count;     // exons of the segment: 1 .. kSegExons
  int32_t slot;      // workspace slot of the segment's partial sums; -1: the row's only segment, written to the output
};

struct Multi {       // a row of more than one segment: its partial sums are the slots slot0 .. slot0 + nseg - 1
  int32_t row;
  int32_t slot0;
  int32_t nseg;
  int32_t pad_;
};

struct Items {
  std::vector<Item> items;
  std::vector<Multi> multi;
  int64_t n_slots = 0;
};

using edrows::row_fault;     // a row against the design: the call form (ed_rows.hpp)

// The items of rows (first[r], last[r]), r = 0 .. n_rows - 1.  Returns 0; 1: a row with first > last or first < 0 (nothing is kept);
// 2: more rows than kMaxRows, or more items than max_items (<= kMaxItems).
inline int build_items(const int32_t* first, const int32_t* last, int64_t n_rows, Items& out, int64_t max_items = kMaxItems)
{
  out = Items();
  if (n_rows < 0 || n_rows > kMaxRows || max_items > kMaxItems) return 2;
  int64_t n_items = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    if (first[r] < 0 || first[r] > last[r]) return 1;
    n_items += n_segments((int64_t)last[r] - first[r] + 1);
    if (n_items > max_items) return 2;
  }
  out.items.reserve((size_t)n_items);
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t n = (int64_t)last[r] - first[r] + 1;
    const int64_t ns = n_segments(n);
    if (ns > 1) out.multi.push_back(Multi{(int32_t)r, (int32_t)out.n_slots, (int32_t)ns, 0});
    for (int64_t j = 0; j < ns; ++j) {
      const int64_t at = j * kSegExons;
      const int64_t cnt = n - at < kSegExons ? n - at : (int64_t)kSegExons;
      out.items.push_back(Item{(int32_t)r, (int32_t)(first[r] + at), (int32_t)cnt, ns > 1 ? (int32_t)(out.n_slots + j) : -1});
    }
    if (ns > 1) out.n_slots += ns;
  }
  return 0;
}

// the plain-double sum of a segment of n values in the kernel's order (the kernel carries a double-double through the same order);
// at(i) is value i of the segment
template <class F>
inline double segment_sum(int n, F at)
{
  double p[kTile];
  for (int l = 0; l < kTile; ++l) p[l] = 0.0;
  for (int i = 0; i < n; ++i) p[i % kTile] += at(i);
  for (int d = kTile / 2; d >= 1; d >>= 1)
    for (int l = 0; l < d; ++l) p[l] += p[l + d];
  return p[0];
}

}  // namespace edratio
