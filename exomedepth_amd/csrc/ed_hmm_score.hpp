// ed_hmm_score.hpp -- derivatives of the HMM's log-transitions with respect to its two parameters, the transition probability t and
// the expected CNV length L.  Host-only: no HIP, no device types; tools/hmm_score_check.cpp checks it stand-alone.
//
// Per gap of distance d (the plan's padded positions, ed_plan_create), f = exp(-d / L):
//   P_A = f/2 + (1 - f)(1 - t)    out of a CNV state into normal         A = log P_A
//   P_B = f/2 + (1 - f) t/2       stay                                   B = log P_B
//   P_C =       (1 - f) t/2       switch deletion <-> duplication        C = log P_C
// and out of normal c0 = log(1 - t), c1 = log(t / 2) whatever the gap.  With f' = df/dL = f d / L^2:
//              d/dt                      d/dL
//   c0     -1 / (1 - t)                   0
//   c1      1 / t                         0
//   A      -(1 - f) / P_A                 f' (t - 1/2) / P_A
//   B       (1 - f) / (2 P_B)             f' (1/2 - t/2) / P_B
//   C       1 / t                        -f' / (1 - f)
// P_C = 0 (a gap of 0, or f rounding to 1): both derivatives of C are 0 -- the entry is -inf for every (t, L) nearby, no path uses it.
// The two padded gaps of a chromosome (the leading one and the closing step) have f' = 0: their distance is 2 L by construction
// (R/class_definition.R:368), so f = exp(-2) up to the integer truncation of the padded position and does not move with L.
//
// The table is laid out as ed_plan::d_lt3 is, per gap and quad lane: lane j reads the log-transitions (l.x, l.y) = (A, A), (B, C),
// (C, B), (A, A) for j = 0 .. 3 and here the four doubles (d/dt l.x, d/dt l.y, d/dL l.x, d/dL l.y) of those two entries.
#pragma once

#include <cmath>
#include <cstdint>

namespace edscore {

constexpr int kRow = 16;   // doubles per gap: 4 quad lanes x 4

struct Gap {               // derivatives of one gap's three entries
  double At, Bt, Ct, AL, BL, CL;
};

// d/dt of the two entries out of normal
inline double dc0_dt(double t) { return -1.0 / (1.0 - t); }
inline double dc1_dt(double t) { return 1.0 / t; }

// `dist` as the plan forms it (double(pos[g + 1]) - double(pos[g])); f with the plan's own expression
inline Gap gap_derivatives(double t, double L, double dist, bool padded)
{
  const double f = std::exp(-dist / L);
  const double g = 1.0 - f;
  const double PA = f * 0.5 + g * (1.0 - t), PB = f * 0.5 + g * (t / 2.0), PC = g * (t / 2.0);
  const double fp = padded ? 0.0 : f * dist / (L * L);
  Gap o;
  o.At = -g / PA;
  o.Bt = g / (2.0 * PB);
  o.AL = fp * (t - 0.5) / PA;
  o.BL = fp * (0.5 - t / 2.0) / PB;
  if (PC > 0.0) {
    o.Ct = 1.0 / t;
    o.CL = (fp == 0.0) ? 0.0 : -fp / g;
  } else {
    o.Ct = 0.0;
    o.CL = 0.0;
  }
  return o;
}

inline void put_row(const Gap& d, double* o)
{
  const double row[kRow] = {d.At, d.At, d.AL, d.AL,    // lane 0: (A, A)
                            d.Bt, d.Ct, d.BL, d.CL,    // lane 1: (B, C)
                            d.Ct, d.Bt, d.CL, d.BL,    // lane 2: (C, B)
                            d.At, d.At, d.AL, d.AL};   // lane 3 shadows lane 0
  for (int i = 0; i < kRow; ++i) o[i] = row[i];
}

// One chromosome of m >= 1 exons: pos[0 .. m + 1] its padded positions, out[(m + 1) * kRow] the rows of its gaps 0 .. m; gaps 0 and
// m are the padded ones.  (An empty chromosome has no gaps and no rows.)
inline void fill_chromosome(double t, double L, const int32_t* pos, int64_t m, double* out)
{
  for (int64_t g = 0; g <= m; ++g) {
    const double dist = double(pos[g + 1]) - double(pos[g]);
    put_row(gap_derivatives(t, L, dist, g == 0 || g == m), out + g * kRow);
  }
}

// The whole table [(E + C)][4][4]: chromosome c's rows start at gap chrom_off[c] + c (as in d_lt3); pad_pos holds the padded positions
// of chromosome c at chrom_off[c] + 2 c.  Rows of gaps no chromosome owns (one per empty chromosome) stay 0.
inline void fill_table(double t, double L, int32_t n_chrom, const int32_t* chrom_off, const int32_t* pad_pos, double* out)
{
  for (int32_t c = 0; c < n_chrom; ++c) {
    const int64_t lo = chrom_off[c], m = (int64_t)chrom_off[c + 1] - lo;
    if (m <= 0) continue;
    fill_chromosome(t, L, pad_pos + lo + 2 * (int64_t)c, m, out + (lo + c) * kRow);
  }
}

}  // namespace edscore
