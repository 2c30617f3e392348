// ratio_plan_check.cpp -- the geometry of the copy-ratio profile (csrc/ed_ratio_plan.hpp) as a stand-alone program, to be run under
// the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o ratio_plan_check tools/ratio_plan_check.cpp && ./ratio_plan_check
//
// It includes only that header.  Over hand-made and seeded sets of rows (lengths on both sides of the tile and of the segment, equal
// rows, overlapping rows, one long row among short ones) it replays the kernel's decode of the items and asserts that
//   every exon of every row is in exactly one item, and an item holds no exon of another row;
//   the items of a row are consecutive, its segments in order, each full but the last, a segment's start a function of the row's length alone;
//   a lane's exons i = t * kTile + lane < count stay inside the segment, and the LDS words of a segment fit kSegExons;
//   rows of one segment have no workspace slot, rows of several own consecutive slots that no other row has, and the Multi list
//   names exactly those rows;
//   the limits are refused: a row with first > last or first < 0, more items than allowed, a grid outside 1 .. kMaxGrid, a dose
//   outside (-2, 2]; row_fault refuses what the interface refuses and nothing else;
//   segment_sum adds every value once (exact on integers) and keeps the documented order (a hand-made case).
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../exomedepth_amd/csrc/ed_ratio_plan.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

uint64_t rng_state = 88172645463325252ull;
uint32_t rnd(uint32_t n)
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

void check_rows(const std::vector<int32_t>& first, const std::vector<int32_t>& last, int32_t E)
{
  using namespace edratio;
  const int64_t n = (int64_t)first.size();
  Items plan;
  CHECK(build_items(first.data(), last.data(), n, plan) == 0);
  std::vector<std::vector<int>> hit((size_t)n);
  for (int64_t r = 0; r < n; ++r) hit[(size_t)r].assign((size_t)(last[r] - first[r] + 1), 0);
  std::vector<int> slot_owner((size_t)plan.n_slots, -1);
  int64_t prev_row = -1, seg = 0, multi_at = 0;
  for (size_t k = 0; k < plan.items.size(); ++k) {
    const Item& it = plan.items[k];
    CHECK(it.row >= 0 && it.row < n);
    CHECK(it.row == prev_row || it.row == prev_row + 1);                 // rows in index order, a row's items consecutive
    seg = it.row == prev_row ? seg + 1 : 0;
    prev_row = it.row;
    const int64_t len = (int64_t)last[it.row] - first[it.row] + 1;
    CHECK(it.count >= 1 && it.count <= kSegExons);
    CHECK(it.first == first[it.row] + seg * kSegExons);                  // where a segment starts follows from the row alone
    CHECK(it.first >= 0 && (int64_t)it.first + it.count - 1 <= last[it.row] && last[it.row] < E);
    CHECK(seg + 1 < n_segments(len) ? it.count == kSegExons : it.count == len - seg * kSegExons);
    // the lanes' decode
    const int nt = n_tiles(it.count);
    CHECK(nt >= 1 && nt <= kSegTiles);
    for (int t = 0; t < nt; ++t)
      for (int lane = 0; lane < kTile; ++lane) {
        const int i = t * kTile + lane;
        if (i >= it.count) continue;
        CHECK(i < kSegExons);
        ++hit[(size_t)it.row][(size_t)(it.first - first[it.row] + i)];
      }
    CHECK((nt - 1) * kTile < it.count);                                  // no tile without an exon
    if (n_segments(len) == 1) {
      CHECK(it.slot == -1);
    } else {
      CHECK(it.slot >= 0 && it.slot < plan.n_slots && slot_owner[(size_t)it.slot] == -1);
      slot_owner[(size_t)it.slot] = it.row;
      if (seg == 0) {
        CHECK(multi_at < (int64_t)plan.multi.size());
        const Multi& m = plan.multi[(size_t)multi_at++];
        CHECK(m.row == it.row && m.slot0 == it.slot && m.nseg == n_segments(len));
      } else {
        CHECK(it.slot == plan.items[k - 1].slot + 1);
      }
    }
  }
  CHECK(prev_row == n - 1);
  CHECK(multi_at == (int64_t)plan.multi.size());
  for (int64_t r = 0; r < n; ++r)
    for (int h : hit[(size_t)r]) CHECK(h == 1);
  for (int o : slot_owner) CHECK(o >= 0);
  // the item limit: one below the need is refused, the need itself is not
  const int64_t need = (int64_t)plan.items.size();
  Items again;
  if (need > 0) CHECK(build_items(first.data(), last.data(), n, again, need - 1) == 2 && again.items.empty());
  CHECK(build_items(first.data(), last.data(), n, again, need) == 0 && (int64_t)again.items.size() == need);
}

void check_limits()
{
  using namespace edratio;
  CHECK(!grid_ok(0) && grid_ok(1) && grid_ok(kMaxGrid) && !grid_ok(kMaxGrid + 1) && !grid_ok(-3));
  CHECK(!dose_ok(-2.0) && dose_ok(-1.9) && dose_ok(0.0) && dose_ok(2.0) && !dose_ok(std::nextafter(2.0, 3.0)) && !dose_ok(NAN) &&
        !dose_ok(HUGE_VAL) && !dose_ok(-HUGE_VAL));
  CHECK(n_segments(1) == 1 && n_segments(kSegExons) == 1 && n_segments(kSegExons + 1) == 2 && n_segments(0) == 0);
  CHECK(n_tiles(1) == 1 && n_tiles(kTile) == 1 && n_tiles(kTile + 1) == 2 && n_tiles(kSegExons) == kSegTiles);
  CHECK(kSegExons * 2 * (int)sizeof(int32_t) * kWaves <= 64 * 1024);      // the parked counts fit static shared memory
  CHECK(kThreads == kWaves * 64 && kTile == 64 && kNarrow >= 0 && kNarrow <= 4);
  Items plan;
  const int32_t f1[] = {3, 7}, l1[] = {5, 6};
  CHECK(build_items(f1, l1, 2, plan) == 1 && plan.items.empty());          // first > last
  const int32_t f2[] = {-1}, l2[] = {4};
  CHECK(build_items(f2, l2, 1, plan) == 1);
  CHECK(build_items(f1, l1, -1, plan) == 2);
  CHECK(build_items(f1, l1, kMaxRows + 1, plan) == 2);
  CHECK(build_items(f1, l1, 0, plan) == 0 && plan.items.empty() && plan.multi.empty() && plan.n_slots == 0);
  const int32_t off[] = {0, 1, 1, 66};                                     // chromosomes of 1, 0 and 65 exons
  CHECK(row_fault(0, 0, 0, 0, 1, 3, off) == 0 && row_fault(6, 2, 1, 65, 7, 3, off) == 0);
  CHECK(row_fault(7, 2, 1, 65, 7, 3, off) == 4 && row_fault(-1, 0, 0, 0, 7, 3, off) == 4);
  CHECK(row_fault(0, 3, 0, 0, 7, 3, off) == 2 && row_fault(0, -1, 0, 0, 7, 3, off) == 2);
  CHECK(row_fault(0, 2, 5, 4, 7, 3, off) == 1);
  CHECK(row_fault(0, 2, 0, 5, 7, 3, off) == 3 && row_fault(0, 2, 1, 66, 7, 3, off) == 3 && row_fault(0, 1, 1, 1, 7, 3, off) == 3 &&
        row_fault(0, 0, 0, 1, 7, 3, off) == 3);
}

void check_sum()
{
  using namespace edratio;
  for (int n : {1, 2, kTile - 1, kTile, kTile + 1, kSegExons - 1, kSegExons}) {
    const double want = 0.5 * n * (n + 1.0);
    CHECK(segment_sum(n, [](int i) { return (double)(i + 1); }) == want);
  }
  std::vector<double> v(kTile + 1, 0.0);
  v[0] = 1e16; v[1] = 1.0; v[32] = -1e16;
  CHECK(segment_sum(kTile + 1, [&](int i) { return v[(size_t)i]; }) == 1.0);   // lanes 0 and 32 meet first
  v[1] = 0.0; v[kTile] = 1.0;
  CHECK(segment_sum(kTile + 1, [&](int i) { return v[(size_t)i]; }) == 0.0);   // value 64 is lane 0's second
}

}  // namespace

int main()
{
  using namespace edratio;
  check_limits();
  check_sum();
  const int T = kTile, S = kSegExons;
  const int32_t E = 4 * S + 100;
  // every length around the tile and the segment, from several starts
  {
    std::vector<int32_t> first, last;
    for (int len : {1, 2, 4, 5, T - 1, T, T + 1, 2 * T, 2 * T + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 7, (int)E})
      for (int32_t at : {0, 1, T - 1, (int)E - len}) {
        if (at < 0 || at + len > E) continue;
        first.push_back(at); last.push_back(at + len - 1);
      }
    check_rows(first, last, E);
    // the same rows in another order, and twice over (equal and overlapping rows)
    std::vector<int32_t> f2(first.rbegin(), first.rend()), l2(last.rbegin(), last.rend());
    f2.insert(f2.end(), first.begin(), first.end()); l2.insert(l2.end(), last.begin(), last.end());
    check_rows(f2, l2, E);
  }
  check_rows({}, {}, E);
  check_rows({0}, {E - 1}, E);
  for (int round = 0; round < 200; ++round) {
    const int n = 1 + (int)rnd(40);
    std::vector<int32_t> first, last;
    for (int r = 0; r < n; ++r) {
      const uint32_t kind = rnd(4);
      const int len = kind == 0 ? 1 + (int)rnd(6) : (kind == 1 ? 1 + (int)rnd(2 * T) : (kind == 2 ? S - 2 + (int)rnd(5) : 1 + (int)rnd((uint32_t)E)));
      const int32_t at = (int32_t)rnd((uint32_t)(E - len + 1));
      first.push_back(at); last.push_back(at + len - 1);
    }
    check_rows(first, last, E);
  }
  std::printf("ratio_plan_check: ok, %ld checks, segments of %d exons\n", n_checks, kSegExons);
  return 0;
}
