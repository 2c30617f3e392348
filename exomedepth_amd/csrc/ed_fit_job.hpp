// ed_fit_job.hpp -- one request to the single-dispersion beta-binomial fit (fit_columns, edfit.inc): which counts, how they lie in memory, where the
// results go and by which method.  Host only: no HIP include, nothing of the library's; edfit.inc takes the request, its checks and the choice of
// histogram geometries from here, and tools/fit_job_check.cpp compiles the same functions into a stand-alone program that runs them under the
// host sanitizers.
#pragma once

#include <cstdint>

// The two selectors below are the kernels' too (fit_hist_runs, edfit.inc): under hipcc they are what they always were, here plain inline functions.
#ifdef __HIPCC__
#define ED_FIT_SEL __host__ __device__ __forceinline__
#else
#define ED_FIT_SEL inline
#endif

// Which geometry serves a batch: depth = the largest per-sample mean total count n (k_fit_start).  The unit bins plus
// the second level of k_fit_hnewton reach n = 9216 / 13312 / 21504; they should cover ~5 x the mean (the synthetic
// design's log-normal exon depths put 99.5 % of the cells below that).  Never a matter of correctness: cells beyond
// the bins are evaluated one by one.
ED_FIT_SEL int fit_hist_geometry(int depth) { return depth <= 1843 ? 8 : (depth <= 2662 ? 4 : 2); }
// Which of the launched geometries runs: fit_columns launches the one the PREVIOUS fit's depth points to (all three
// the first time), `launched` says which (bit 0 / 1 / 2 = 8 / 4 / 2 samples per workgroup).  If the data's own choice
// is among them it runs; if not (the depth changed between calls) the launched geometry with the longest bins does --
// every geometry gives the same answer, only the time differs.
ED_FIT_SEL int fit_hist_bit(int ks) { return ks == 8 ? 1 : (ks == 4 ? 2 : 4); }

// the two error codes a refused request carries: ED_ERR_INVALID and ED_ERR_STATE of include/exomedepth_amd.h (edfit.inc asserts the equality)
constexpr int kFitJobErrInvalid = -1;
constexpr int kFitJobErrState = -5;

// Column s of the fit has test counts test[e * trs + (tmod ? s % tmod : s) * tcs] and reference counts ref[e * rrs + s], e < E -- or, sample-major
// (sm_pitch > 0), it is the row test[s * sm_pitch + e * trs], ref likewise.  Four layouts mean something; the constructors below are the only
// way to a job, so there is no fifth.
struct FitJob {
  enum View { kExonMajor, kSampleMajor, kSharedTest, kCyclicTest };
  View view;
  const int32_t* test;
  const int32_t* ref;
  int64_t trs, tcs, rrs;         // test row / column stride, reference row stride (elements)
  int64_t tmod = 0;              // kCyclicTest: column s takes test column s mod tmod
  int64_t sm_pitch = 0;          // kSampleMajor: elements between consecutive samples' rows
  int cb = 4;                    // bytes per count (2: uint16 matrices, sample-major only)
  int skip_K = 0;                // kCyclicTest: prefixes per test column, closed early by k_fit_skip_prefixes ...
  int* d_skip_from = nullptr;    // ... which leaves the first prefix it closed here, [tmod]
  int64_t E = 0, S = 0;          // rows and columns of THIS fit
  double* phi = nullptr;         // [S] device outputs
  double* expected = nullptr;
  int hist = 0;                  // 0: per-cell passes; 1: count histograms, geometry chosen from the data; 8 / 4 / 2: that geometry
  int mode = 0;                  // 0: maximum likelihood (Newton); 1: aod-nm

  // [E][S] matrices, one column per sample; by > 1: every by-th row (subset.for.speed)
  static FitJob exon_major(const int32_t* test, const int32_t* ref, int64_t S, int64_t by = 1) { return FitJob(kExonMajor, test, S * by, 1, ref, S * by); }
  // [S][E] matrices, `pitch` counts between samples, every by-th exon, cb bytes per count
  static FitJob sample_major(const int32_t* test, const int32_t* ref, int64_t pitch, int64_t by, int cb)
  {
    FitJob j(kSampleMajor, test, by, 1, ref, by);
    j.sm_pitch = pitch; j.cb = cb;
    return j;
  }
  // ONE test column against each of the R columns of ref ([E][R]): select.reference.set's prefixes
  static FitJob shared_test(const int32_t* test, const int32_t* ref, int64_t R) { return FitJob(kSharedTest, test, 1, 0, ref, R); }
  // T test columns ([E][T]) against R = K * T reference columns ([E][R]), column i * T + j being test j against its i + 1 best candidates summed
  // (edrefcohort.inc); d_skip_from: see k_fit_skip_prefixes
  static FitJob cyclic_test(const int32_t* test, int64_t T, const int32_t* ref, int64_t R, int K, int* d_skip_from)
  {
    FitJob j(kCyclicTest, test, T, 1, ref, R);
    j.tmod = T; j.skip_K = K; j.d_skip_from = d_skip_from;
    return j;
  }

  FitJob& over(int64_t E_, int64_t S_) { E = E_; S = S_; return *this; }                        // E rows x S columns
  FitJob& into(double* d_phi, double* d_expected) { phi = d_phi; expected = d_expected; return *this; }
  FitJob& by_method(int hist_, int mode_ = 0) { hist = hist_; mode = mode_; return *this; }

  bool sample_major() const { return view == kSampleMajor; }
  bool column_per_sample() const { return view == kExonMajor || view == kSampleMajor; }   // test laid out like ref: what the histogram kernels read

 private:
  FitJob(View v, const int32_t* t, int64_t trs_, int64_t tcs_, const int32_t* r, int64_t rrs_) : view(v), test(t), ref(r), trs(trs_), tcs(tcs_), rrs(rrs_) {}
};

namespace fitjob {

// Why job j cannot be served by a workspace made for work_E rows x work_S columns (0 x 0: never allocated): the message and *code, or NULL.
// Nothing has been enqueued when fit_columns asks.
inline const char* invalid(const FitJob& j, int64_t work_E, int64_t work_S, int* code)
{
  *code = kFitJobErrState;
  if (j.cb != 4 && !j.sample_major())
    return "fit: 16-bit counts (ed_batch_set_counts_bits(batch, 16)) are fitted from sample-major matrices only (counts_layout 1)";
  if (j.sample_major() && !j.hist)
    return "fit: sample-major counts are fitted on the count histograms only (ed_batch_set_fit_histograms(batch, 0) excludes them)";
  if (j.mode == 1 && !j.hist)
    return "fit mode 1 (aod-nm) works on the count histograms: ed_batch_set_fit_histograms(batch, 0) excludes it";
  // The partials, (eta, lam, done), the packed column map and the histograms are all sized by the workspace's own (E, S).  No caller gets here:
  //  - ed_batch_fit_subset, edbins.inc (twice) and edcov.inc use the batch's workspace, made by batch_fitwork(b, E, S) for the plan's E and the batch's S,
  //    and fit those or (subset.for.speed) fewer rows;
  //  - edrefset.inc allocates a workspace for exactly its (n, Rw) in the lines before the call;
  //  - edrefcohort.inc takes RcScratch::fit_work(n, R), which regrows the kept workspace whenever either dimension exceeds what it has.
  if (work_E < j.E || work_S < j.S || work_S <= 0)
    return "fit: the workspace is smaller than the fit (or was never allocated)";
  *code = kFitJobErrInvalid;
  if (j.hist && !j.column_per_sample()) return "fit_columns: histogram path needs per-sample test columns";
  return nullptr;
}

// Which histogram geometries to launch (bits as fit_hist_bit): the one asked for (tests), else the one the previous fit's depth `hint` points to,
// else (hint < 0: first fit of the workspace) all three.
inline int launched_geometries(int hist, int hint)
{
  return hist > 1 ? fit_hist_bit(hist) : (hint < 0 ? 7 : fit_hist_bit(fit_hist_geometry(hint)));
}

}   // namespace fitjob
