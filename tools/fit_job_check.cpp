// fit_job_check.cpp -- the request of the dispersion fit (csrc/ed_fit_job.hpp) as a stand-alone program, to be run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o fit_job_check tools/fit_job_check.cpp && ./fit_job_check
//
// It includes only that header.  The four constructors against the strides fit_columns took positionally before there was a FitJob, the five
// refusals (each on a minimal job, with its text and code) against every accepted job of the callers' table, the launched-geometries mask on both
// sides of its two depth thresholds, and the workspace bound at equality and one below.
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../exomedepth_amd/csrc/ed_fit_job.hpp"

namespace {

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

int32_t counts[4];             // never read: the job only carries the addresses
double outs[2];
int skip[1];
const int32_t* const T = counts;
const int32_t* const R = counts + 2;

bool strides(const FitJob& j, int64_t trs, int64_t tcs, int64_t rrs, int64_t tmod, int64_t pitch, int cb, int skip_K, const int* skip_from)
{
  return j.test == T && j.ref == R && j.trs == trs && j.tcs == tcs && j.rrs == rrs && j.tmod == tmod && j.sm_pitch == pitch && j.cb == cb &&
         j.skip_K == skip_K && j.d_skip_from == skip_from;
}

// refused with exactly this text and code
bool refused(const FitJob& j, int64_t work_E, int64_t work_S, const char* text, int code)
{
  int c = 0;
  const char* why = fitjob::invalid(j, work_E, work_S, &c);
  return why && std::strcmp(why, text) == 0 && c == code;
}
bool accepted(const FitJob& j, int64_t work_E, int64_t work_S)
{
  int c = 0;
  return fitjob::invalid(j, work_E, work_S, &c) == nullptr;
}

const char* const kMsg16 = "fit: 16-bit counts (ed_batch_set_counts_bits(batch, 16)) are fitted from sample-major matrices only (counts_layout 1)";
const char* const kMsgSm = "fit: sample-major counts are fitted on the count histograms only (ed_batch_set_fit_histograms(batch, 0) excludes them)";
const char* const kMsgNm = "fit mode 1 (aod-nm) works on the count histograms: ed_batch_set_fit_histograms(batch, 0) excludes it";
const char* const kMsgCols = "fit_columns: histogram path needs per-sample test columns";
const char* const kMsgWork = "fit: the workspace is smaller than the fit (or was never allocated)";

void constructors()
{
  CHECK(strides(FitJob::exon_major(T, R, 70), 70, 1, 70, 0, 0, 4, 0, nullptr));
  CHECK(strides(FitJob::exon_major(T, R, 70, 3), 210, 1, 210, 0, 0, 4, 0, nullptr));
  CHECK(strides(FitJob::sample_major(T, R, 2100, 1, 4), 1, 1, 1, 0, 2100, 4, 0, nullptr));
  CHECK(strides(FitJob::sample_major(T, R, 2100, 3, 2), 3, 1, 3, 0, 2100, 2, 0, nullptr));
  CHECK(strides(FitJob::shared_test(T, R, 9), 1, 0, 9, 0, 0, 4, 0, nullptr));
  CHECK(strides(FitJob::cyclic_test(T, 12, R, 132, 11, skip), 12, 1, 132, 12, 0, 4, 11, skip));
  const FitJob j = FitJob::exon_major(T, R, 70).over(2100, 70).into(outs, outs + 1).by_method(8, 1);
  CHECK(j.E == 2100 && j.S == 70 && j.phi == outs && j.expected == outs + 1 && j.hist == 8 && j.mode == 1);
  const FitJob d = FitJob::shared_test(T, R, 9);
  CHECK(d.E == 0 && d.S == 0 && d.phi == nullptr && d.expected == nullptr && d.hist == 0 && d.mode == 0);
  CHECK(FitJob::exon_major(T, R, 1).column_per_sample() && FitJob::sample_major(T, R, 1, 1, 4).column_per_sample());
  CHECK(!FitJob::shared_test(T, R, 1).column_per_sample() && !FitJob::cyclic_test(T, 1, R, 1, 1, skip).column_per_sample());
}

void refusals()
{
  // the callers' table: every job of it passes, with a workspace of exactly its size
  for (int hist : {0, 1, 8, 4, 2}) CHECK(accepted(FitJob::exon_major(T, R, 70).over(2100, 70).by_method(hist), 2100, 70));
  CHECK(accepted(FitJob::exon_major(T, R, 70, 3).over(700, 70).by_method(1), 2100, 70));
  CHECK(accepted(FitJob::exon_major(T, R, 5).over(300, 5).by_method(1, 1), 300, 5));
  for (int cb : {4, 2})
    for (int64_t by : {1, 3}) CHECK(accepted(FitJob::sample_major(T, R, 2100, by, cb).over(2100 / by, 70).by_method(1), 2100, 70));
  CHECK(accepted(FitJob::sample_major(T, R, 300, 1, 4).over(300, 5).by_method(4, 1), 300, 5));
  CHECK(accepted(FitJob::shared_test(T, R, 9).over(2100, 9), 2100, 9));
  CHECK(accepted(FitJob::cyclic_test(T, 12, R, 132, 11, skip).over(2100, 132), 2100, 132));

  // 16-bit counts outside the sample-major view
  FitJob j16 = FitJob::exon_major(T, R, 3).over(64, 3).by_method(1);
  j16.cb = 2;
  CHECK(refused(j16, 64, 3, kMsg16, kFitJobErrState));
  FitJob s16 = FitJob::shared_test(T, R, 3).over(64, 3);
  s16.cb = 2;
  CHECK(refused(s16, 64, 3, kMsg16, kFitJobErrState));
  // a sample-major view without histograms (also in fit mode 1: this refusal comes first, as it did)
  CHECK(refused(FitJob::sample_major(T, R, 64, 1, 4).over(64, 3).by_method(0), 64, 3, kMsgSm, kFitJobErrState));
  CHECK(refused(FitJob::sample_major(T, R, 64, 1, 2).over(64, 3).by_method(0, 1), 64, 3, kMsgSm, kFitJobErrState));
  // fit mode 1 without histograms
  CHECK(refused(FitJob::exon_major(T, R, 3).over(64, 3).by_method(0, 1), 64, 3, kMsgNm, kFitJobErrState));
  // histograms on a view that is not one column per sample
  CHECK(refused(FitJob::shared_test(T, R, 3).over(64, 3).by_method(1), 64, 3, kMsgCols, kFitJobErrInvalid));
  CHECK(refused(FitJob::cyclic_test(T, 3, R, 6, 2, skip).over(64, 6).by_method(8), 64, 6, kMsgCols, kFitJobErrInvalid));
  // a workspace that is too small, or was never allocated
  const FitJob ok = FitJob::exon_major(T, R, 3).over(64, 3).by_method(1);
  CHECK(accepted(ok, 64, 3));
  CHECK(accepted(ok, 65, 4));
  CHECK(refused(ok, 63, 3, kMsgWork, kFitJobErrState));
  CHECK(refused(ok, 64, 2, kMsgWork, kFitJobErrState));
  CHECK(refused(ok, 0, 0, kMsgWork, kFitJobErrState));
  CHECK(refused(FitJob::exon_major(T, R, 0).over(0, 0), 0, 0, kMsgWork, kFitJobErrState));   // (nothing allocated serves nothing, not even an empty fit)
  const FitJob pc = FitJob::shared_test(T, R, 3).over(64, 3);
  CHECK(accepted(pc, 64, 3) && refused(pc, 63, 3, kMsgWork, kFitJobErrState) && refused(pc, 64, 2, kMsgWork, kFitJobErrState));
}

void mask()
{
  CHECK(fit_hist_bit(8) == 1 && fit_hist_bit(4) == 2 && fit_hist_bit(2) == 4);
  CHECK(fit_hist_geometry(0) == 8 && fit_hist_geometry(1843) == 8 && fit_hist_geometry(1844) == 4);
  CHECK(fit_hist_geometry(2662) == 4 && fit_hist_geometry(2663) == 2 && fit_hist_geometry(2000000000) == 2);
  CHECK(fitjob::launched_geometries(1, -1) == 7);          // first fit of a workspace: all three
  CHECK(fitjob::launched_geometries(1, 0) == 1);
  CHECK(fitjob::launched_geometries(1, 1843) == 1);
  CHECK(fitjob::launched_geometries(1, 1844) == 2);
  CHECK(fitjob::launched_geometries(1, 2662) == 2);
  CHECK(fitjob::launched_geometries(1, 2663) == 4);
  for (int hint : {-1, 0, 1843, 1844, 2662, 2663}) {       // a forced geometry, whatever the hint
    CHECK(fitjob::launched_geometries(8, hint) == 1);
    CHECK(fitjob::launched_geometries(4, hint) == 2);
    CHECK(fitjob::launched_geometries(2, hint) == 4);
  }
}

}  // namespace

int main()
{
  constructors();
  refusals();
  mask();
  std::printf("fit job: %ld checks ok\n", n_checks);
  return 0;
}
