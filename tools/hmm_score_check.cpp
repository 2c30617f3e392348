// hmm_score_check.cpp -- the table of the log-transitions' derivatives (csrc/ed_hmm_score.hpp) as a stand-alone program, to be run under
// the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o hmm_score_check tools/hmm_score_check.cpp && ./hmm_score_check
//
// It includes only that header.  Every entry of a gap's derivatives against central differences (step 1e-4 theta) of the long-double
// log-probabilities, over four settings of (t, L) and distances from 0 to 1e8; the special cases (P_C = 0 at a distance of 0, f = 0 at
// 1e8, the padded gaps whose f does not move with L); the layout of whole tables (lane order, the rows of an empty chromosome, a
// chromosome of one exon whose gaps are both padded) against the per-gap function.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../exomedepth_amd/csrc/ed_hmm_score.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

typedef long double ld;

// log P of entry `which` (0 A, 1 B, 2 C, 3 c0, 4 c1) at (t, L); a padded gap keeps the f of L0
ld logp(int which, ld t, ld L, double dist, bool padded, ld L0)
{
  const ld f = std::exp(-(ld)dist / (padded ? L0 : L));
  const ld g = 1.0L - f;
  switch (which) {
    case 0: return std::log(f / 2 + g * (1 - t));
    case 1: return std::log(f / 2 + g * t / 2);
    case 2: return std::log(g * t / 2);
    case 3: return std::log(1 - t);
    default: return std::log(t / 2);
  }
}

double worst = 0.0;

// `got` against the central difference along theta (0: t, 1: L); the allowance is 1e-6 of the value plus the rounding of the difference
void against_difference(double got, int which, int theta, double t, double L, double dist, bool padded)
{
  const ld h = 1e-4L * (theta ? (ld)L : (ld)t);
  const ld hi = theta ? logp(which, t, (ld)L + h, dist, padded, L) : logp(which, (ld)t + h, L, dist, padded, L);
  const ld lo = theta ? logp(which, t, (ld)L - h, dist, padded, L) : logp(which, (ld)t - h, L, dist, padded, L);
  const ld fd = (hi - lo) / (2 * h);
  const ld mag = std::fabs(logp(which, t, L, dist, padded, L));
  const ld tol = 1e-6L * std::fabs(fd) + 8 * LDBL_EPSILON * (mag > 1 ? mag : 1) / h;
  const ld err = std::fabs((ld)got - fd);
  CHECK(err <= tol);
  if (fd != 0) { const double r = (double)(err / std::fabs(fd)); if (r > worst && std::fabs(fd) > 1e-12) worst = r; }
}

void check_gap(double t, double L, double dist, bool padded)
{
  const edscore::Gap d = edscore::gap_derivatives(t, L, dist, padded);
  const double f = std::exp(-dist / L);
  const double got[3][2] = {{d.At, d.AL}, {d.Bt, d.BL}, {d.Ct, d.CL}};
  for (int which = 0; which < 3; ++which) {
    if (which == 2 && (1.0 - f) * (t / 2.0) == 0.0) {      // P_C = 0: the entry is -inf and has no derivative; the table says 0
      CHECK(d.Ct == 0.0 && d.CL == 0.0);
      continue;
    }
    for (int theta = 0; theta < 2; ++theta) {
      CHECK(std::isfinite(got[which][theta]));
      against_difference(got[which][theta], which, theta, t, L, dist, padded);
    }
  }
  if (padded) CHECK(d.AL == 0.0 && d.BL == 0.0 && d.CL == 0.0);
  if (f == 0.0) CHECK(d.AL == 0.0 && d.BL == 0.0 && d.CL == 0.0);      // the rows equal the from-normal row, which does not know L
  against_difference(edscore::dc0_dt(t), 3, 0, t, L, dist, padded);
  against_difference(edscore::dc1_dt(t), 4, 0, t, L, dist, padded);
}

// whole tables: the plan's padded positions of a layout, rows against the per-gap function, lane by lane
void check_table(double t, double L)
{
  const int sizes[] = {1, 0, 3, 17, 0, 2};
  const int C = (int)(sizeof sizes / sizeof sizes[0]);
  std::vector<int32_t> chrom_off(C + 1, 0);
  for (int c = 0; c < C; ++c) chrom_off[c + 1] = chrom_off[c] + sizes[c];
  const int E = chrom_off[C];
  std::vector<int32_t> start(E), end(E);
  for (int c = 0; c < C; ++c) {
    int32_t x = 1000000;
    for (int i = chrom_off[c]; i < chrom_off[c + 1]; ++i) {
      const int k = i - chrom_off[c];
      x += (k == 3) ? 0 : ((k == 5) ? 100000000 : 137 * (k + 1) + 40 * c);     // a gap of 0 and one of 1e8 in the long chromosome
      start[i] = x;
      end[i] = x + 90;
    }
  }
  std::vector<int32_t> pad((size_t)E + 2 * C, -7);
  for (int c = 0; c < C; ++c) {
    const int lo = chrom_off[c], m = sizes[c];
    if (m <= 0) continue;
    int32_t* p = pad.data() + lo + 2 * c;
    p[0] = (int32_t)((double)start[lo] - 2 * L);
    for (int i = 0; i < m; ++i) p[1 + i] = start[lo + i];
    p[m + 1] = (int32_t)((double)end[lo + m - 1] + 2 * L);
  }
  const double mark = -12345.0;
  std::vector<double> tab((size_t)(E + C) * edscore::kRow, mark);
  edscore::fill_table(t, L, C, chrom_off.data(), pad.data(), tab.data());
  std::vector<char> owned(E + C, 0);
  for (int c = 0; c < C; ++c) {
    const int lo = chrom_off[c], m = sizes[c];
    if (m <= 0) continue;
    const int32_t* p = pad.data() + lo + 2 * c;
    for (int g = 0; g <= m; ++g) {
      const bool padded = (g == 0 || g == m);
      const double dist = double(p[g + 1]) - double(p[g]);
      const edscore::Gap d = edscore::gap_derivatives(t, L, dist, padded);
      const double* r = tab.data() + (size_t)(lo + c + g) * edscore::kRow;
      owned[lo + c + g] = 1;
      const double want[16] = {d.At, d.At, d.AL, d.AL, d.Bt, d.Ct, d.BL, d.CL, d.Ct, d.Bt, d.CL, d.BL, d.At, d.At, d.AL, d.AL};
      for (int i = 0; i < 16; ++i) CHECK(r[i] == want[i]);
      if (padded) for (int lane = 0; lane < 4; ++lane) CHECK(r[lane * 4 + 2] == 0.0 && r[lane * 4 + 3] == 0.0);
      if (!padded) check_gap(t, L, dist, false);
    }
    if (m == 1) {                                            // every gap of the chain is padded: nothing moves with L
      for (int g = 0; g <= 1; ++g)
        for (int lane = 0; lane < 4; ++lane) {
          const double* r = tab.data() + (size_t)(lo + c + g) * edscore::kRow + lane * 4;
          CHECK(r[2] == 0.0 && r[3] == 0.0);
        }
    }
  }
  int untouched = 0;
  for (int g = 0; g < E + C; ++g)
    if (!owned[g]) {                                         // an empty chromosome: its one row is nobody's and is not written
      ++untouched;
      for (int i = 0; i < edscore::kRow; ++i) CHECK(tab[(size_t)g * edscore::kRow + i] == mark);
    }
  CHECK(untouched == 2);
}

}  // namespace

int main()
{
  const double settings[][2] = {{1e-4, 50000.0}, {0.01, 20000.0}, {0.04, 6000.0}, {0.3, 300.0}};
  const double dists[] = {0.0, 1.0, 100.0, 137.0, 5000.0, 9000.0, 123456.0, 1e6, 1e8};
  for (const auto& s : settings) {
    for (double d : dists)
      for (int padded = 0; padded < 2; ++padded) check_gap(s[0], s[1], d, padded != 0);
    check_gap(s[0], s[1], 2 * s[1], true);                   // a padded gap as the plan makes it
    check_table(s[0], s[1]);
  }
  // an empty design: no chromosome, nothing written
  {
    const int32_t off[1] = {0};
    double none[1] = {3.0};
    edscore::fill_table(1e-4, 50000.0, 0, off, nullptr, none);
    CHECK(none[0] == 3.0);
  }
  std::printf("hmm_score_check: ok, %ld checks, largest relative difference to a central difference %.3g\n", n_checks, worst);
  return 0;
}
