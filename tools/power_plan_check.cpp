// power_plan_check.cpp -- the geometry of the detection-power map (csrc/ed_power_plan.hpp) as a stand-alone program, to be run under
// the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o power_plan_check tools/power_plan_check.cpp && ./power_plan_check
//
// It includes only that header and asserts that
//   a total is valid exactly on 0 .. kMaxTotal; the word and the bit of every valid total lie inside a row of the map that map_words gives
//   for any largest total at or above it, the narrow map below the occupancy cap and the wide one from it on;
//   the job layout of any set of per-sample job counts (zeros, ties, one long sample) is a permutation: every (sample, k) with
//   k < count[s] gets a place of its own inside 0 .. n_jobs, all jobs k stand before all jobs k + 1;
//   the walk's tiles cover x = 0 .. n and no more than a tile beyond;
//   region_sum adds every value of a run exactly once (exact on integers) and keeps the documented order (a hand-made case);
//   row_fault refuses what the interface refuses and nothing else; the gaps a price reads lie inside the chromosome's rows of the table.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../exomedepth_amd/csrc/ed_power_plan.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

void check_totals()
{
  using namespace edpower;
  CHECK(kMaxTotal >= (1 << 20));
  CHECK(!total_ok(-1) && total_ok(0) && total_ok(kMaxTotal) && !total_ok((int64_t)kMaxTotal + 1) && !total_ok((int64_t)1 << 40));
  const int32_t probes[] = {0, 1, 31, 32, 33, kOccCap - 1, kOccCap, kOccCap + 1, kMaxTotal - 1, kMaxTotal};
  for (int32_t largest : probes) {
    const int32_t words = map_words(largest);
    CHECK(words == (largest < kOccCap ? kOccCap / 32 : kMaxTotal / 32 + 1));
    for (int32_t n : probes) {
      if (n > largest) continue;
      CHECK(word_of(n) >= 0 && word_of(n) < words);
      CHECK(below_mask(n) == ((n & 31) ? (0xffffffffu >> (32 - (n & 31))) : 0u));
    }
  }
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)254, (int64_t)255, (int64_t)256, (int64_t)1023, (int64_t)1024, (int64_t)kMaxTotal}) {
    const int64_t nt = n_walk_tiles(n);
    CHECK(nt * kWalkTile >= n + 1 && (nt - 1) * kWalkTile < n + 1);
  }
}

void check_jobs(const std::vector<int32_t>& count)
{
  const int64_t S = (int64_t)count.size();
  const edpower::JobLayout L = edpower::job_layout(count.data(), S);
  int64_t total = 0;
  int32_t most = 0;
  for (int32_t c : count) { total += c; most = c > most ? c : most; }
  CHECK(L.n_jobs == total && L.max_jobs == most && (int64_t)L.off_k.size() == (int64_t)most + 1 && (int64_t)L.rank.size() == S);
  std::vector<int32_t> key((size_t)total, -1);
  for (int64_t s = 0; s < S; ++s)
    for (int32_t k = 0; k < count[(size_t)s]; ++k) {
      const int64_t j = L.off_k[(size_t)k] + L.rank[(size_t)s];
      CHECK(j >= 0 && j < total);
      CHECK(key[(size_t)j] == -1);
      key[(size_t)j] = k;
    }
  for (int64_t j = 0; j < total; ++j) {
    CHECK(key[(size_t)j] >= 0);
    if (j) CHECK(key[(size_t)j - 1] <= key[(size_t)j]);
  }
}

void check_region_sum()
{
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)513, (int64_t)4096}) {
    std::vector<int> seen((size_t)n, 0);
    const double s = edpower::region_sum(n, [&](int64_t i) { seen[(size_t)i] += 1; return (double)(i + 1); });
    CHECK(s == (double)(n * (n + 1) / 2));
    for (int v : seen) CHECK(v == 1);
  }
  // the order: lanes 0 and 32 meet first.  1e16 + 1 loses the 1; (1e16 + -1e16) + (1 + 0) keeps it
  const double v[65] = {1e16, 1.0};
  std::vector<double> run(v, v + 65);
  run[32] = -1e16;
  CHECK(edpower::region_sum(65, [&](int64_t i) { return run[(size_t)i]; }) == 1.0);
  run[32] = 0.0; run[64] = -1e16;        // value 64 is lane 0's second: (1e16 + -1e16) first, then + 1
  CHECK(edpower::region_sum(65, [&](int64_t i) { return run[(size_t)i]; }) == 1.0);
  run[1] = 0.0; run[64] = 1.0; run[32] = -1e16;      // the 1 is lane 0's second value: 1e16 + 1 loses it before lane 32 comes in
  CHECK(edpower::region_sum(65, [&](int64_t i) { return run[(size_t)i]; }) == 0.0);
}

void check_rows()
{
  const int32_t off[] = {0, 5, 5, 6, 20};          // chromosome 1 is empty, chromosome 2 has one exon
  const int32_t C = 4;
  CHECK(edpower::row_fault(0, 0, 4, C, off) == 0 && edpower::row_fault(2, 5, 5, C, off) == 0 && edpower::row_fault(3, 6, 19, C, off) == 0);
  CHECK(edpower::row_fault(0, 3, 2, C, off) == 1);
  CHECK(edpower::row_fault(-1, 0, 0, C, off) == 2 && edpower::row_fault(4, 0, 0, C, off) == 2);
  CHECK(edpower::row_fault(0, 3, 5, C, off) == 3);          // across the boundary
  CHECK(edpower::row_fault(1, 5, 5, C, off) == 3);          // an empty chromosome holds no run
  CHECK(edpower::row_fault(3, 5, 7, C, off) == 3 && edpower::row_fault(3, 19, 20, C, off) == 3 && edpower::row_fault(0, -1, 2, C, off) == 3);
  for (int32_t c = 0; c < C; ++c) {
    const int32_t lo = off[c], m = off[c + 1] - off[c];
    for (int32_t a = 0; a < m; ++a)
      for (int32_t b = a; b < m; ++b) {
        const edpower::PriceGaps g = edpower::price_gaps(lo + a, lo + b, c);
        const int64_t row0 = (int64_t)lo + c, row1 = row0 + m;      // the chromosome's rows of the table: gaps 0 .. m
        CHECK(g.n_nn == b - a + 2);
        CHECK(g.inner1 - g.inner0 == b - a && g.inner0 > row0 && g.inner1 <= row1);
        CHECK(g.close == g.inner1 && g.close <= row1);
      }
  }
}

}  // namespace

int main()
{
  check_totals();
  check_jobs({});
  check_jobs({0});
  check_jobs({1});
  check_jobs({3, 0, 3, 1, 7, 0, 2, 2});
  check_jobs({5, 5, 5, 5});
  check_jobs({0, 0, 1000, 0});
  {
    std::vector<int32_t> c;
    for (int i = 0; i < 300; ++i) c.push_back((i * 37) % 23);
    check_jobs(c);
  }
  check_region_sum();
  check_rows();
  std::printf("power_plan_check: ok, %ld checks\n", n_checks);
  return 0;
}
