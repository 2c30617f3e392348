// quant_plan_check.cpp -- the rules of the quantile map (csrc/ed_quant_plan.hpp) as a stand-alone program, to be run under the host
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o quant_plan_check tools/quant_plan_check.cpp && ./quant_plan_check
//
// It includes only that header and asserts that
//   a list of probabilities is valid exactly when it has 1 .. kMaxProbs entries, all finite, inside (0, 1) and strictly ascending, and
//   every fault gets its own code;
//   cut_of gives the cut back from q = cut + f for every fraction 0 < f < 1 -- cut = 0 (q = p / pm[0]) included --, names the value below
//   a whole q (the tie C(q - 1) = p), is 0 at and below 0 and kNoCut for NaN and for what no count can reach;
//   bin_of counts the cuts at or below a count: bins closed below, a count on a cut in the upper bin, equal cuts crossed together, a
//   missing cut (kNoCut) above every count.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../exomedepth_amd/csrc/ed_quant_plan.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

void check_probs()
{
  using edquant::probs_fault;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double band[] = {0.025, 0.975};
  CHECK(probs_fault(band, 2) == 0 && probs_fault(band, 1) == 0);
  CHECK(probs_fault(nullptr, 2) == 1 && probs_fault(band, 0) == 1 && probs_fault(band, -1) == 1);
  std::vector<double> many;
  for (int k = 0; k < edquant::kMaxProbs + 1; ++k) many.push_back((k + 1) / 32.0);
  CHECK(probs_fault(many.data(), edquant::kMaxProbs) == 0 && probs_fault(many.data(), edquant::kMaxProbs + 1) == 1);
  const double bad_nan[] = {0.1, nan}, bad_inf[] = {0.1, inf}, zero[] = {0.0, 0.5}, one[] = {0.5, 1.0}, neg[] = {-0.1}, above[] = {1.5};
  CHECK(probs_fault(bad_nan, 2) == 2 && probs_fault(bad_inf, 2) == 2);
  CHECK(probs_fault(zero, 2) == 3 && probs_fault(one, 2) == 3 && probs_fault(neg, 1) == 3 && probs_fault(above, 1) == 3);
  const double same[] = {0.5, 0.5}, down[] = {0.975, 0.025};
  CHECK(probs_fault(same, 2) == 4 && probs_fault(down, 2) == 4);
  const double tight[] = {0.5, std::nextafter(0.5, 1.0), 1.0 - 0x1p-53};
  CHECK(probs_fault(tight, 3) == 0);
  const double tiny[] = {std::numeric_limits<double>::denorm_min()};
  CHECK(probs_fault(tiny, 1) == 0);
}

void check_cuts()
{
  using edquant::cut_of;
  using edquant::kNoCut;
  for (int64_t cut : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)4099, (int64_t)1 << 20}) {
    for (double f : {0x1p-30, 0.25, 0.5, 0.999}) CHECK(cut_of((double)cut + f) == cut);
    CHECK(cut_of(std::nextafter((double)cut + 1.0, 0.0)) == cut);
    CHECK(cut_of((double)cut + 1.0) == cut);              // a whole q: the value below it
    if (cut > 0) CHECK(cut_of(std::nextafter((double)cut, 1e300)) == cut);
  }
  CHECK(cut_of(std::numeric_limits<double>::denorm_min()) == 0);
  CHECK(cut_of(0.0) == 0 && cut_of(-0.0) == 0 && cut_of(-3.5) == 0);
  CHECK(cut_of(std::numeric_limits<double>::quiet_NaN()) == kNoCut);
  CHECK(cut_of(std::numeric_limits<double>::infinity()) == kNoCut && cut_of(0x1p53) == kNoCut && cut_of(0x1p53 - 1.0) == ((int64_t)1 << 53) - 2);
}

void check_bins()
{
  using edquant::bin_of;
  const int64_t cuts[] = {3, 7, 7, 20};
  CHECK(bin_of(0, cuts, 4) == 0 && bin_of(2, cuts, 4) == 0);
  CHECK(bin_of(3, cuts, 4) == 1 && bin_of(6, cuts, 4) == 1);         // on a cut: the upper bin
  CHECK(bin_of(7, cuts, 4) == 3 && bin_of(19, cuts, 4) == 3);        // equal cuts are crossed together: the bin between them stays empty
  CHECK(bin_of(20, cuts, 4) == 4 && bin_of((int64_t)1 << 40, cuts, 4) == 4);
  const int64_t none[] = {0, edquant::kNoCut};
  CHECK(bin_of(0, none, 2) == 1 && bin_of((int64_t)1 << 40, none, 2) == 1);      // a cut at 0 is below every count, a missing one above
  CHECK(bin_of(5, cuts, 0) == 0);
  // every count lands in exactly one of the K + 1 bins, and the bins ascend with the count
  int last = 0;
  for (int64_t obs = 0; obs < 30; ++obs) {
    const int b = bin_of(obs, cuts, 4);
    CHECK(b >= last && b <= 4);
    last = b;
  }
}

}  // namespace

int main()
{
  check_probs();
  check_cuts();
  check_bins();
  std::printf("quant_plan_check: ok, %ld checks\n", n_checks);
  return 0;
}
