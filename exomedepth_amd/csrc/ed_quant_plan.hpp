// ed_quant_plan.hpp -- the rules of the quantile map that are not arithmetic on the device (csrc/edquant.inc).  Host-only:
// no HIP, no device types; tools/quant_plan_check.cpp checks it stand-alone.  The kernels read the constants and the constexpr functions.
// The occupancy map, the job list, the walk's tiles and the order of a region's sums are the detection-power map's (ed_power_plan.hpp).
//
// Probabilities.  A request names 1 .. kMaxProbs probabilities, finite, inside (0, 1) and strictly ascending: the walk crosses them in
// that order and ends at the last.
// Cut.  For a probability p, cut = the smallest x with C(x) > p (C = the running sum of the masses) and
//   q = cut + (p - C(cut - 1)) / pm[cut]        (C(-1) = 0: for cut = 0 this is p / pm[0]),
// so q lies in [cut, cut + 1), and in (cut, cut + 1) unless C(cut - 1) = p exactly.  cut_of(q) = ceil(q) - 1 gives the cut back from every
// q that is not a whole number -- for cut = 0 as well: q = p / pm[0] lies in (0, 1), ceil(q) - 1 = 0.  A whole q is the tie C(q - 1) = p:
// cut_of names the value below, q - 1, the cell whose upper end G(q) = C(q - 1) = p is -- the convention of G, which is closed above.  No
// quantile (NaN: nothing crossed) has no cut: kNoCut, above every count.
// Bins.  K probabilities cut the counts 0 .. n into K + 1 bins; the bin of an observed count is the number of k with obs >= cut_k: bins are
// closed below, a count equal to a cut belongs to the upper bin, as C(x) > p dictates.
#pragma once

#include <cmath>
#include <cstdint>

namespace edquant {

constexpr int kMaxProbs = 16;
constexpr int64_t kNoCut = INT64_MAX;

// 0: a valid list; 1: not 1 .. kMaxProbs entries (or no list); 2: an entry that is not finite; 3: an entry outside (0, 1);
// 4: not strictly ascending
inline int probs_fault(const double* probs, int64_t n)
{
  if (!probs || n < 1 || n > kMaxProbs) return 1;
  for (int64_t k = 0; k < n; ++k) {
    if (!std::isfinite(probs[k])) return 2;
    if (!(probs[k] > 0.0 && probs[k] < 1.0)) return 3;
    if (k > 0 && !(probs[k] > probs[k - 1])) return 4;
  }
  return 0;
}

// (ceil without <cmath>: the kernels call this too.  q < 2^53 wherever a count can be)
constexpr int64_t cut_of(double q)
{
  if (!(q == q) || q >= 0x1p53) return kNoCut;
  if (!(q > 0.0)) return 0;
  const int64_t t = (int64_t)q;               // q > 0: truncation is floor
  return (double)t == q ? t - 1 : t;          // ceil(q) - 1
}

constexpr int bin_of(int64_t obs, const int64_t* cuts, int n_cuts)
{
  int b = 0;
  for (int k = 0; k < n_cuts; ++k) b += obs >= cuts[k] ? 1 : 0;
  return b;
}

}  // namespace edquant
