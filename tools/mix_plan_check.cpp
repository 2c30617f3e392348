// mix_plan_check.cpp -- the launch geometry of the mixture profile (csrc/ed_mix_plan.hpp) as a stand-alone program, to be run under
// the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o mix_plan_check tools/mix_plan_check.cpp && ./mix_plan_check
//
// It includes only that header.  Over small designs (chromosome lengths on both sides of the tile, empty chromosomes, equal lengths),
// widths S and grids G = 1 .. 16 it replays the launch -- workgroup (x, y) serves pair x and chromosome job_chrom[y], quad q of its chain
// wave the grid point quad_grid(q, G) if quad_live(q, G) -- and asserts that
//   every (pair, non-empty chromosome, grid point) is stored exactly once, an empty chromosome never;
//   the launch rows come longest first, ties in index order;
//   the tiles of a chain are disjoint, inside the chain, in order, and cover it; a tile's rows fit the buffer;
//   every column of a tile's row has exactly one owner and lies inside the row;
//   the bytes of LDS stay within the limit of static shared memory.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../exomedepth_amd/csrc/ed_mix_plan.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

void check_tiles(int m)
{
  const int nt = edmix::n_tiles(m);
  CHECK(nt >= 1);
  int next = 0;
  for (int t = 0; t < nt; ++t) {
    const int first = edmix::tile_first(t), cnt = edmix::tile_count(m, t);
    CHECK(first == next);
    CHECK(cnt >= 1 && cnt <= edmix::kTile);
    CHECK(first >= 0 && first + cnt <= m);                      // every exon a lane loads lies inside the chain
    if (t + 1 < nt) CHECK(cnt == edmix::kTile);
    CHECK((cnt - 1) * edmix::kRowStride + edmix::kRowStride <= edmix::kTile * edmix::kRowStride);
    next = first + cnt;
  }
  CHECK(next == m);
  CHECK(edmix::tile_first(nt) >= m);
}

void check_columns(int G)
{
  const int nc = edmix::n_cols(G);
  CHECK(nc >= 3 && nc <= edmix::kRowStride);
  std::vector<int> owner(nc, 0);
  ++owner[0];                                                   // the normal state
  for (int g = 0; g < G; ++g) {
    CHECK(edmix::col_del(g) > 0 && edmix::col_del(g) < nc);
    CHECK(edmix::col_dup(g) > 0 && edmix::col_dup(g) < nc);
    ++owner[edmix::col_del(g)];
    ++owner[edmix::col_dup(g)];
  }
  for (int c = 0; c < nc; ++c) CHECK(owner[c] == 1);
  // the emission waves' passes: wave w takes columns w, w + kEmitWaves, ...: every column once
  std::vector<int> passes(nc, 0);
  for (int w = 0; w < edmix::kEmitWaves; ++w)
    for (int c = w; c < nc; c += edmix::kEmitWaves) ++passes[c];
  for (int c = 0; c < nc; ++c) CHECK(passes[c] == 1);
  // the quads of the chain wave
  std::vector<int> stores(G, 0);
  for (int q = 0; q < edmix::kMaxGrid; ++q) {
    const int g = edmix::quad_grid(q, G);
    CHECK(g >= 0 && g < G);                                     // a shadowing quad reads columns that exist
    if (edmix::quad_live(q, G)) ++stores[g];
  }
  for (int g = 0; g < G; ++g) CHECK(stores[g] == 1);
}

void check_design(const std::vector<int>& sizes, int S, int G)
{
  const int32_t C = (int32_t)sizes.size();
  std::vector<int32_t> off((size_t)C + 1, 0);
  for (int32_t c = 0; c < C; ++c) off[c + 1] = off[c] + sizes[c];
  const std::vector<int32_t> jobs = edmix::job_order(C, off.data());
  int nonempty = 0;
  for (int m : sizes) nonempty += m > 0;
  CHECK((int)jobs.size() == nonempty);
  for (size_t y = 0; y + 1 < jobs.size(); ++y) {
    const int a = sizes[jobs[y]], b = sizes[jobs[y + 1]];
    CHECK(a > b || (a == b && jobs[y] < jobs[y + 1]));
  }
  std::vector<int> hit((size_t)S * C * G, 0);
  for (int32_t y = 0; y < (int32_t)jobs.size(); ++y)
    for (int64_t x = 0; x < S; x += edmix::kPairsPerWg) {
      const edmix::Job job = edmix::job_of(x, y, jobs);
      CHECK(job.pair >= 0 && job.pair < S && job.chrom >= 0 && job.chrom < C);
      CHECK(sizes[job.chrom] > 0);
      for (int q = 0; q < edmix::kMaxGrid; ++q)
        if (edmix::quad_live(q, G)) ++hit[((size_t)edmix::quad_grid(q, G) * C + job.chrom) * S + job.pair];
    }
  for (int g = 0; g < G; ++g)
    for (int32_t c = 0; c < C; ++c)
      for (int s = 0; s < S; ++s) CHECK(hit[((size_t)g * C + c) * S + s] == (sizes[c] > 0 ? 1 : 0));
}

}  // namespace

int main()
{
  CHECK(edmix::lds_bytes() <= edmix::kLdsLimit);
  CHECK(edmix::lds_bytes() >= 2 * edmix::kTile * edmix::n_cols(edmix::kMaxGrid) * 8);
  CHECK(edmix::kRowStride >= edmix::n_cols(edmix::kMaxGrid) && edmix::kRowStride % 2 == 1);
  CHECK(edmix::kThreads % 64 == 0 && edmix::kEmitWaves >= 1 && edmix::kTile <= 64 && edmix::kPairsPerWg == 1);
  const int T = edmix::kTile;
  for (int m = 1; m <= 4 * T + 7; ++m) check_tiles(m);
  check_tiles(200000);
  for (int G = 1; G <= edmix::kMaxGrid; ++G) check_columns(G);
  const std::vector<std::vector<int>> designs = {
    {}, {0}, {1}, {0, 0}, {1, 2, T, 0, 3 * T + 5}, {0, 1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5},
    {5, 5, 5}, {T, 0, T, 2 * T, 0, T}, {3, 9, 1, 9, 0, 2}};
  for (const auto& d : designs)
    for (int S : {1, 3, 17})
      for (int G = 1; G <= edmix::kMaxGrid; ++G) check_design(d, S, G);
  std::printf("mix_plan_check: ok, %ld checks, %d bytes of LDS a workgroup\n", n_checks, edmix::lds_bytes());
  return 0;
}
