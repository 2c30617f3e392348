// edtab.inc -- the table-driven emission mode (ed_batch_set_emit_mode(batch, 1)).  Included by edcore.hip.
//
// What it replaces: the per-cell evaluation of  log B(a1 + obs, a2 + tot - obs) - log B(a1, a2)  (reference
// src/CNV_estimate.cpp:44-50 -> src/beta.c:49-114) through GSL's routes -- ~1 140 binary64 lane-instructions per cell in
// k_emit_batch, which reproduces GSL operation for operation -- by the identity the reference itself states at
// src/beta.c:101-108, log B(x, y) = lgamma(x) + lgamma(y) - lgamma(x + y):
//     emission = D(a1, obs) + D(a2, ref) - D(a1 + a2, tot),   D(x, k) = lgamma(x + k) - lgamma(x) = sum_{i<k} log(x + i)
// (ref = tot - obs: the reference-sample count).  Per (sample, state) the three D(., k) are tables over the count ranges of
// the sample (ed_dtab.h: double-double prefix sums of a double-double logarithm, rounded once per entry); a cell is three
// gathers and a compensated three-term sum.  Results agree with the reference to ~1e-14 relative (the north star asks for
// 1e-10 on log-likelihoods and identical Viterbi paths); the strict kernel stays the default and the verifier
// (ed_batch_verify_emissions_tol).
//
//   k_tab_stats   subsampled pass over the counts: per-sample sum of test / reference counts -> table lengths
//   tab_dims_of   per sample: (Ly, Lr) = lengths of the obs / ref tables (the tot table has Ly + Lr entries); 0 = the sample's
//                 parameters are outside what the tables serve (GSL error, non-positive shape, ill-conditioned sum): strict
//   k_tab_build   per (sample, table): the entries of the three states, by a workgroup-wide double-double scan
//   k_emit_tab    per cell: gathers + sum; cells outside their sample's tables are appended to a list
//   k_tab_cold    the listed cells through the strict arithmetic (edsf::lnbeta: the reference's routes, same bits as mode 0)
//
// Layout of one sample's tables: entries of 3 doubles (deletion, normal, duplication -- the states share the counts, so one
// gather serves all three), T1 at entry 0 (Ly entries, index obs), T2 at Ly (Lr entries, index ref), T3 at Ly + Lr
// (Ly + Lr entries, index tot); samples `stride` entries apart.

// A slab's preparation kernels (k_tab_stats_sm, k_tab_build) are the emission stream's critical path, yet run at the default wave priority: 3 against 0,
// with the Viterbi kernel at 0 or 3, measured equal (4.08-4.18 / 4.04-4.13 / 4.08-4.24 ms per step) -- wave priority
// arbitrates issue slots, and these kernels wait for memory and for each other's registers, not for issue slots.
namespace {

// Counts on the device: int32 (R's integers; cb = 4) or, in the sample-major table mode only (ed_batch_set_counts_bits(batch, 16)), uint16 (cb = 2: counts
// below 65 536, half the bytes of every pass over them).  `base` is the matrix' first element either way; i an element index.
__device__ __forceinline__ int32_t ed_ldc(const int32_t* __restrict__ base, int64_t i, int cb)
{
  return cb == 2 ? (int32_t)reinterpret_cast<const uint16_t*>(base)[i] : base[i];
}

constexpr int kTabBlock = 256;
// Cells outside their sample's tables are appended to kColdLists lists, each with its own counter (cold_n[i], i < kColdLists; a
// wave picks its list from its workgroup number): one counter for the whole launch was the same-address atomic of ~5e5 waves per slab.
// cold_n[kColdLists] is raised when a list ran out: the strict pass then looks at every cell of the launch again.
constexpr int kColdLists = 1024;

// per-sample sums over a sample of the exons -- every `step`-th piece of 64 consecutive exons (so that the sample-major form below
// reads whole 256-byte pieces and both forms look at the SAME exons: the table lengths, hence which cells take the strict
// arithmetic, do not depend on the layout the counts arrive in): acc [3][S] = sum of test counts, of reference counts, rows seen
__global__ void __launch_bounds__(256)
k_tab_stats(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t E, int64_t S, int step,
            unsigned long long* __restrict__ acc)
{
  __shared__ unsigned long long red[3][4][64];
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 64 + lane;
  const int64_t e0 = (int64_t)blockIdx.y * 64 * step + sub * 16;     // this workgroup's piece: exons [y 64 step, y 64 step + 64)
  unsigned long long sy = 0, sr = 0, n = 0;
  if (s < S) {
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int64_t e = e0 + k;
      if (e < E) {
        const int32_t y = test[e * S + s], r = ref[e * S + s];
        sy += (unsigned long long)(y > 0 ? y : 0);
        sr += (unsigned long long)(r > 0 ? r : 0);
        n += 1;
      }
    }
  }
  red[0][sub][lane] = sy; red[1][sub][lane] = sr; red[2][sub][lane] = n;
  __syncthreads();
  if (sub == 0 && s < S) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const unsigned long long v = red[q][0][lane] + red[q][1][lane] + red[q][2][lane] + red[q][3][lane];
      if (v) atomicAdd(&acc[(int64_t)q * S + s], v);   // integer sums: the same whatever the order
    }
  }
}

// the same from sample-major counts [S][E] (`pitch` ints between samples): four ONE-WAVE workgroups per sample (blockIdx.y: which quarter of the
// pieces), every `step`-th 64-exon piece; integer sums added atomically into acc (zeroed by k_sample_consts) -- one-wave workgroups are placed
// wherever a SIMD has room, a four-wave one waits for a CU with room on all four (this kernel heads the next slab's preparation beside a running
// Viterbi launch: 0.72 ms for 0.04 ms of work in round 5's trace)
__global__ void __launch_bounds__(64)
k_tab_stats_sm(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t pitch, int64_t E, int64_t S, int step,
               unsigned long long* __restrict__ acc, int cb)
{
  const int lane = threadIdx.x, wave = blockIdx.y;
  const int64_t s = blockIdx.x;
  unsigned long long sy = 0, sr = 0, n = 0;
  for (int64_t q = (int64_t)wave * step; q * 64 < E; q += 4 * step) {
    const int64_t e = q * 64 + lane;
    if (e < E) {
      const int32_t y = ed_ldc(test, s * pitch + e, cb), r = ed_ldc(ref, s * pitch + e, cb);
      sy += (unsigned long long)(y > 0 ? y : 0);
      sr += (unsigned long long)(r > 0 ? r : 0);
      n += 1;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { sy += __shfl_xor(sy, d, 64); sr += __shfl_xor(sr, d, 64); n += __shfl_xor(n, d, 64); }
  if (lane == 0) {
    if (sy) atomicAdd(&acc[s], sy);
    if (sr) atomicAdd(&acc[S + s], sr);
    if (n) atomicAdd(&acc[2 * S + s], n);
  }
}

// Table lengths of every sample, and which of its cells the tables serve.  A table reaches `reach` x the sample's mean count
// (+ 64): the log-normal exon depths of exome data put > 99.8 % of the cells below 8 x the mean, and what lies beyond goes
// through the strict arithmetic.  dims[s] = (Ly, Lr, Tm1, reason):
//   Ly, Lr   lengths of the obs / ref tables; a cell is served when obs < Ly, ref < Lr (its tot then lies inside the tot table)
//   Tm1      cells with 0 < tot <= Tm1 are NOT served (strict list); 0 = every cell is
//   w        a sample WITH tables: N0 -- cells with ref = 0 and obs >= N0 are not served (0x7fffffff = every such cell is);
//            a sample without: the reason, see below
//   reason   why the sample has none (Ly = Lr = 0: the WHOLE sample goes through the strict arithmetic in
//            one dedicated pass of k_tab_cold): 1 a per-sample constant raised a GSL error, 2 a shape parameter is not a positive
//            normal number (phi >= 1, expected outside (0, 1), ...: the reference's error paths and reflection branches live in
//            the strict code only), 3 the three-term sum is ill conditioned at any useful length, 4 too many of its cells fall
//            under the few-reads rule for a list
// Eligibility is per CELL wherever the arithmetic allows it (round 4 excluded whole samples: in the reference's own workflow --
// aggregate references of 20 - 32 samples, expected ~0.03 -- that sent most of a cohort through the strict lists):
//   - Conditioning of the three-term sum.  The entries are correctly rounded, so a cell's value carries at most
//     2^-53 (|D1| + |D2| + |D3|) <= 2^-52 n log(a12 + n) of absolute error (n = tot), and log E[p^obs (1 - p)^ref] decreases in both
//     counts, so |value| >= min(a1, a2) log(1 + n / (2 a12)) (the value at (n / 2, 0) or (0, n / 2) bounds it and
//     -log(1 - u) >= u).  The ratio grows with n: the tables are CUT at the length where it reaches 3e-11 (a third of the bar)
//     instead of refusing the sample -- cells beyond the cut are ordinary out-of-table cells.  Round 4's rule had no logarithm in
//     the denominator and the whole-sample granularity; with min(a1, a2) ~ 1 - 2 (deletion state of a deep reference) it fired
//     where the real ratio is 5 - 9e-12.
//   - Few reads under a nearly binomial model (a1 + a2 > 2e3, phi < 5e-4 .. 8e-4): there the REFERENCE's value is the difference
//     of two log-Betas of size ~(a1 + a2) H(expected), each carrying ~eps (a1 + a2) log(a1 + a2) of absolute error on the
//     log-gamma route (src/beta.c:101-108), against a value of ~tot |log(1 - p)|: measured 8.8e-11 relative at a12 = 4.3e3,
//     (obs, ref) = (0, 1), i.e. ~2.4e-15 a12 log(a12) / tot.  The tables are the more accurate of the two, but parity is measured
//     against the reference: cells with 0 < tot < a12 log(a12) / 15200 (= 1 at a12 = 2e3, the limit measured at 2.7e-11 in 9.6e8
//     cells; 51 at a12 = 7e4) take the strict arithmetic.  Cells without reads are exact on both sides (0 = c - c).
//   - The reference's second argument.  src/CNV_estimate.cpp:49 forms it as (a2 + total) - observed: two roundings, the first at the
//     size of the TOTAL, so the argument carries up to 2^-53 (a2 + tot) of absolute error whatever is left after the subtraction;
//     the log-Beta moves by |psi(y) - psi(x + y)| times that.  For y = a2 + ref >= 1 this is another ~2^-53 n log(a12 + n), folded
//     into the conditioning bound (its factor 2^-51 instead of 2^-52).  For ref = 0 and a small a2 (expected close to 1: the test
//     sample deeper than its reference) psi(y) ~ -1 / a2 and the value itself is only ~a2 log(1 + n / a12): found by
//     tools/fuzz_tables.py at a2 = 1.5e-3, (obs, ref) = (24, 0) -- the reference 2.1e-10 away from the exact value, the tables 2e-12.
//     Cells with ref = 0 and obs >= N0 take the strict arithmetic (= the reference's roundings), N0 the first n where
//     2^-53 (a2 + n) (1 / a2 + log(a12 + n) + 1) exceeds 3e-11 a2 log(1 + n / a12) in some state; exome data (a2 >> 1): none.
constexpr double kTabCondBar = 3e-11;       // conditioning: the tables are cut where the bound on the relative error reaches this
constexpr double kTabFewReads = 15200.0;    // few-reads rule: tot >= a12 log(a12) / this
__device__ __forceinline__ double tab_cond_bound(double a12, double amin, double n)
{
  const double x = n / (2.0 * a12);
  const double lg = x > 1e-6 ? ed_plog(1.0 + x) : x;
  return 0x1p-51 * n * ed_plog(a12 + n) / (amin * lg);
}
// ref = 0: bound on (the reference's error from its rounded second argument) / |value| at obs = n
__device__ __forceinline__ double tab_ref0_bound(double a12, double a2, double n)
{
  const double x = n / a12;
  const double lg = x > 1e-6 ? ed_plog(1.0 + x) : x;
  return 0x1p-53 * (a2 + n) * (1.0 / a2 + ed_plog(a12 + n) + 1.0) / (a2 * lg);
}
// ---- the sample-major form's LDS windows, and the samples whose counts outgrow them (round 6) ------------------------------------------------
// A workgroup of the sample-major emission kernel keeps kSmEntries table entries in LDS: the first n1 of the obs table, n2 of the ref table, n3 of the tot
// table (tab_windows).  Up to a depth of ~250 reads per exon and test sample (aggregate references 8 x deeper) 70 - 90 % of the cells find all three of
// their entries there and the rest fetch theirs from the tables in global memory (L2).  Deeper data turn the kernel into that gather (depth 400: 2.2 x the
// time per cell, depth 1 600: 7 x, with the tables at their length caps and a sixth of the cells on the strict lists -- extra.regimes of the bench line,
// round 5's state).  A sample whose mean total count reaches kTailMeanOverWindow x its tot window is therefore a TAIL sample: its tables are built for the
// windows only, every index beyond a window is served by Stirling's series (ed_dtab.h: ed_dtab_tail: one logarithm, a division and a dozen fma per state
// and term, whatever the count), and its cells are served up to the conditioning limit instead of up to a table length -- a branch of the emission kernel
// (emit_tail_share, a branch of k_emit_tab_sm taken per workgroup) walks the tail samples.  Which samples are tail samples is decided from the same subsampled statistics as
// the table lengths: by the data alone, not by the launch history.
constexpr int kSmEntries = 6144;          // table entries a workgroup keeps in LDS (x 24 B = 147 456 B)
constexpr int kSmT1Max = 1024;            // ... at most this many of them from the obs table
constexpr double kTailMeanOverWindow = 1.25;
constexpr int kTailMaxCount = 1 << 24;    // tail samples: obs + ref below this (the limit of the conditioning search)

__device__ __forceinline__ int4 tab_windows(int Ly, int Lr, int tail)
{
  const int n1 = Ly < kSmT1Max ? Ly : kSmT1Max;
  int n2 = (kSmEntries - n1) / 2;
  if (n2 > Lr) n2 = Lr;
  int n3 = kSmEntries - n1 - n2;
  if (n3 > Ly + Lr) n3 = Ly + Lr;
  return make_int4(n1, n2, n3, tail);
}
// conditioning bound where the series serves: it forms lgamma(z) whole, so what it can keep is an ulp of (a12 + n) log(a12 + n), not of the difference
// (tests/test_dtab.py); twice the table bound's constant for its ~1 ulp against the tables' half
__device__ __forceinline__ double tab_cond_bound_tail(double a12, double amin, double n)
{
  const double x = n / (2.0 * a12);
  const double lg = x > 1e-6 ? ed_plog(1.0 + x) : x;
  return 0x1p-50 * (a12 + n) * ed_plog(a12 + n) / (amin * lg);
}

__device__ __forceinline__ int4 tab_dims_of(const double* __restrict__ consts, const int* __restrict__ cflags,
                                            const unsigned long long* __restrict__ acc, int64_t S, int64_t s, double reach, int capY, int capR,
                                            int tails = 0, int4* __restrict__ win = nullptr)
{
  const double n = (double)acc[2 * S + s];
  const double my = n > 0 ? (double)acc[s] / n : 0.0, mr = n > 0 ? (double)acc[S + s] / n : 0.0;
  int Ly = (int)fmin(reach * my + 64.0, (double)capY), Lr = (int)fmin(reach * mr + 64.0, (double)capR);
  Ly = (Ly + 7) & ~7; Lr = (Lr + 7) & ~7;
  if (Ly > capY) Ly = capY;
  if (Lr > capR) Lr = capR;
  double a12s[3], amins[3], a2s[3];
  int reason = 0;
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    const double a1 = consts[(st * 3 + 0) * S + s], a2 = consts[(st * 3 + 1) * S + s], a12 = a1 + a2;
    if (reason == 0 && cflags[st * S + s] != 0) reason = 1;
    if (reason == 0 && !(ed_dtab_shape_ok(a1) && ed_dtab_shape_ok(a2) && ed_dtab_shape_ok(a12))) reason = 2;
    a12s[st] = a12; amins[st] = fmin(a1, a2); a2s[st] = a2;
  }
  if (win) *win = make_int4(0, 0, 0, 0);
  if (reason) return make_int4(0, 0, 0, reason);
  // a tail sample?  (the windows its natural table lengths give; the bound must hold where the windows end -- the tables' part -- and where the series
  //  starts; the served counts then reach as far as the series' bound allows: it falls, then rises with n, so its two ends say it all)
  bool tail = false;
  if (tails) {
    const int4 w0 = tab_windows(Ly, Lr, 1);
    bool ok = (my + mr) >= kTailMeanOverWindow * (double)w0.z && w0.x >= ED_DTAB_TAIL_FROM && w0.y >= ED_DTAB_TAIL_FROM && w0.z >= ED_DTAB_TAIL_FROM;
#pragma unroll
    for (int st = 0; st < 3; ++st)
      ok = ok && tab_cond_bound(a12s[st], amins[st], (double)(w0.x + w0.y)) <= kTabCondBar && tab_cond_bound_tail(a12s[st], amins[st], (double)w0.y) <= kTabCondBar;
    if (ok) {
      int lo = w0.x + w0.y, hi = kTailMaxCount;      // bound(lo) holds; the largest n <= hi at which it does
      bool top = true;
#pragma unroll
      for (int st = 0; st < 3; ++st) top = top && tab_cond_bound_tail(a12s[st], amins[st], (double)hi) <= kTabCondBar;
      if (!top) {
        while (hi - lo > 8) {
          const int mid = lo + ((hi - lo) >> 1);
          bool okm = true;
#pragma unroll
          for (int st = 0; st < 3; ++st) okm = okm && tab_cond_bound_tail(a12s[st], amins[st], (double)mid) <= kTabCondBar;
          if (okm) lo = mid; else hi = mid;
        }
      } else lo = hi;
      // the served counts: obs < Ly, ref < Lr with Ly + Lr = that limit, dealt in proportion to the sample's mean counts (both at least their windows)
      const double share = mr / fmax(my + mr, 1.0);
      int nLr = (int)fmin(fmax((double)lo * share, (double)w0.y), (double)(lo - w0.x)) & ~7;
      int nLy = (lo - nLr) & ~7;
      if (nLy >= w0.x && nLr >= w0.y) { Ly = nLy; Lr = nLr; tail = true; if (win) *win = w0; }
    }
  }
  // conditioning: shorten the longer table (by an eighth at a time, multiples of 8) until the bound holds in every state
  if (!tail) {
#pragma unroll 1
  for (int it = 0; it < 64; ++it) {
    const double nn = (double)(Ly + Lr);
    bool ok = true;
#pragma unroll
    for (int st = 0; st < 3; ++st) ok = ok && tab_cond_bound(a12s[st], amins[st], nn) <= kTabCondBar;
    if (ok) break;
    if (Ly <= 64 && Lr <= 64) return make_int4(0, 0, 0, 3);
    if (Lr >= Ly) { Lr = (Lr - (Lr >> 3)) & ~7; if (Lr < 64) Lr = 64; }
    else { Ly = (Ly - (Ly >> 3)) & ~7; if (Ly < 64) Ly = 64; }
  }
  {
    bool ok = true;
#pragma unroll
    for (int st = 0; st < 3; ++st) ok = ok && tab_cond_bound(a12s[st], amins[st], (double)(Ly + Lr)) <= kTabCondBar;
    if (!ok) return make_int4(0, 0, 0, 3);
  }
  if (win) *win = tab_windows(Ly, Lr, 0);
  }
  // few reads under a nearly binomial model
  double tmin = 0.0;
#pragma unroll
  for (int st = 0; st < 3; ++st)
    if (a12s[st] > 2e3) tmin = fmax(tmin, ceil(a12s[st] * ed_plog(a12s[st]) / kTabFewReads));
  if (tmin > 1.0 && 4.0 * tmin > my + mr) { if (win) *win = make_int4(0, 0, 0, 0); return make_int4(0, 0, 0, 4); }     // (a tenth of a log-normal sample's cells or more: not list material)
  const int Tm1 = tmin > 1.0 ? (int)fmin(tmin - 1.0, 2147483000.0) : 0;
  // ref = 0 with a small a2: the first obs at which the reference's own rounding comes too close to the bar (bisection: the bound grows with n)
  int N0 = 0x7fffffff;
#pragma unroll 1
  for (int st = 0; st < 3; ++st) {
    if (tab_ref0_bound(a12s[st], a2s[st], (double)(Ly - 1)) <= kTabCondBar) continue;
    int lo = 0, hi = Ly - 1;             // bound(lo) holds (lo = 0: no reads, exact), bound(hi) does not
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tab_ref0_bound(a12s[st], a2s[st], (double)mid) <= kTabCondBar) lo = mid; else hi = mid;
    }
    if (hi < N0) N0 = hi;
  }
  return make_int4(Ly, Lr, Tm1, N0);
}
// what the emission kernels and the strict pass agree on: the cell's emissions come from its sample's tables
__device__ __forceinline__ bool tab_cell_served(int32_t obs, int32_t nref, int Ly, int Lr, int Tm1, int N0)
{
  return (unsigned)obs < (unsigned)Ly && (unsigned)nref < (unsigned)Lr && !((unsigned)obs + (unsigned)nref - 1u < (unsigned)Tm1) &&
         !(nref == 0 && obs >= N0);
}

__device__ __forceinline__ ed_dd dd_shfl_up(ed_dd v, int d)
{
  return ed_dd_make(__shfl_up(v.hi, d, 64), __shfl_up(v.lo, d, 64));
}

// One workgroup per (sample, table): entries k = 1 .. L-1 are the prefix sums of log(x0 + i), i < k, in double-double
// (ed_dtab.h).  Per sweep (one state at a time) a thread evaluates kTabRun16 consecutive logarithms and sums them locally; a wave
// scan of the threads' totals (shuffles) and an LDS step across the four waves give every thread the sum of everything before
// it; a running double-double carries the total from sweep to sweep.  (16 entries per thread: with 4 the scan -- 10 double-double
// additions and 14 shuffles per thread and sweep -- cost three times the logarithms.)  The association of the additions differs
// from the sequential definition's: to ~2^-100, i.e. the same entries after rounding.
constexpr int kTabPer = 16;
// Workgroups of ONE wave (round 5; 256 threads before): the kernel runs next to k_viterbi_sm's persistent grid and the next slab's fit, and
// a one-wave workgroup is placed wherever a SIMD has registers left, while a four-wave one waits for a CU with room on all four; the scan
// across waves (an LDS step and a barrier per state and sweep) goes away with them.  A sweep now covers 64 x 16 = 1 024 entries.
// (A batch of few samples has few tables to build and the chip to itself: there the four-wave form finishes the long tot table sooner --
// tab_build launches it below 256 samples.)
template <int kTabBuildBlock>
__global__ void __launch_bounds__(kTabBuildBlock)
k_tab_build(const double* __restrict__ consts, const int* __restrict__ cflags, const unsigned long long* __restrict__ acc, double reach, int capY,
            int capR, int4* __restrict__ dims, int64_t S, double* __restrict__ tabs, int64_t stride, unsigned int* __restrict__ notab,
            int tails = 0, int4* __restrict__ wins = nullptr, double* __restrict__ lg0 = nullptr)
{
  constexpr int kTabBuildWaves = kTabBuildBlock / 64;
  __shared__ double s_logt[ED_PM_LOGT_N * 3];
  __shared__ ed_dd wtot[3][kTabBuildWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < ED_PM_LOGT_N * 3; i += kTabBuildBlock) s_logt[i] = (&k_logt_rows[0][0])[i];
  const int64_t s = blockIdx.x;
  const int t = blockIdx.y;
  int4 w;
  const int4 d = tab_dims_of(consts, cflags, acc, S, s, reach, capY, capR, tails, &w);    // (every workgroup of the sample works them out: no launch of its own)
  if (t == 0 && tid == 0) {
    dims[s] = d;
    if (wins) wins[s] = w;
    if (d.x == 0) notab[1u + atomicAdd(notab, 1u)] = (unsigned int)s;          // samples without tables: notab[0] of them, listed behind it
    else if (w.w) notab[(S + 2) + atomicAdd(notab + (S + 1), 1u)] = (unsigned int)s;     // tail samples: notab[S + 1] of them, listed behind it (a statistic: ed_batch_table_stats)
  }
  // a tail sample's tables end with its LDS windows (and sit back to back); the others' reach their served lengths
  const int L = w.w ? ((t == 0) ? w.x : ((t == 1) ? w.y : w.z)) : ((t == 0) ? d.x : ((t == 1) ? d.y : d.x + d.y));
  const int64_t tb = w.w ? ((t == 0) ? 0 : ((t == 1) ? w.x : w.x + w.y)) : ((t == 0) ? 0 : ((t == 1) ? d.x : d.x + d.y));
  if (L <= 0) return;
  double* __restrict__ out = tabs + (s * stride + tb) * 3;
  if (tid < 3) out[tid] = 0.0;       // D(x, 0) = 0
  __syncthreads();
  double x0s[3];
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    const double a1 = consts[(st * 3 + 0) * S + s], a2 = consts[(st * 3 + 1) * S + s];
    x0s[st] = (t == 0) ? a1 : ((t == 1) ? a2 : a1 + a2);
  }
  if (w.w && lg0 && tid < 3) {        // log Gamma of the table's shape parameter, what the series subtracts: [S][3 tables][3 states] (hi, lo)
    const ed_dd g = ed_dtab_lg0(tid == 0 ? x0s[0] : (tid == 1 ? x0s[1] : x0s[2]), s_logt);
    double* o = lg0 + ((s * 3 + t) * 3 + tid) * 2;
    o[0] = g.hi; o[1] = g.lo;
  }
  ed_dd carry[3] = {ed_dd_make(0, 0), ed_dd_make(0, 0), ed_dd_make(0, 0)};
  // The three states of a sweep are finished before anything is stored: a thread then holds its 16 consecutive ENTRIES whole
  // (48 doubles = 384 contiguous bytes) and a wave 24 contiguous KB, written once.  (State by state, every line of a table was
  // written three times, 8 bytes in every 24: the L2 cannot hold a workgroup's 240 KB until the next state comes round, so each
  // pass went to memory as partial lines -- WRITE_SIZE 1.40 GB per 1024 samples for 0.48 GB of tables.)
#pragma unroll 1
  for (int base = 0; base < L - 1; base += kTabBuildBlock * kTabPer) {
    const int i0 = base + tid * kTabPer;
    double val[kTabPer][3];
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      const double x0 = x0s[st];
      ed_dd pre[kTabPer];
      ed_dd run = ed_dd_make(0, 0);
      if (i0 < L - 1) {                // (threads beyond the table's end add nothing)
#pragma unroll
        for (int j = 0; j < kTabPer; ++j) {
          run = ed_dd_add_fast(run, ed_ddlog_t(x0 + (double)(i0 + j), s_logt));
          pre[j] = run;
        }
      }
      ed_dd inc = run;                 // inclusive scan of the threads' totals inside the wave
#pragma unroll
      for (int dd = 1; dd < 64; dd <<= 1) {
        const ed_dd o = dd_shfl_up(inc, dd);
        if (lane >= dd) inc = ed_dd_add(o, inc);
      }
      ed_dd exc = dd_shfl_up(inc, 1);  // what the threads before this one (in the wave) add up to
      if (lane == 0) exc = ed_dd_make(0, 0);
      ed_dd before = carry[st], all = carry[st];
      if (kTabBuildWaves > 1) {
        if (lane == 63) wtot[st][wave] = inc;
        __syncthreads();               // (wtot[st] is next written a sweep later, two barriers after its last reader)
#pragma unroll
        for (int w = 0; w < kTabBuildWaves; ++w) {
          if (w < wave) before = ed_dd_add(before, wtot[st][w]);
          all = ed_dd_add(all, wtot[st][w]);
        }
      } else {
        all = ed_dd_add(all, ed_dd_make(__shfl(inc.hi, 63, 64), __shfl(inc.lo, 63, 64)));   // the wave's total: lane 63's inclusive sum
      }
      carry[st] = all;
      before = ed_dd_add(before, exc);
      if (i0 < L - 1) {
#pragma unroll
        for (int j = 0; j < kTabPer; ++j) val[j][st] = ed_dd_add_hi(before, pre[j]);
      }
    }
    // entry k = i0 + j + 1 holds the logarithms 0 .. k-1; the thread's entries are contiguous
    if (i0 < L - 1) {
      double* __restrict__ o = out + (int64_t)(i0 + 1) * 3;
      if (i0 + kTabPer < L) {
#pragma unroll
        for (int j = 0; j < kTabPer; ++j) { o[3 * j] = val[j][0]; o[3 * j + 1] = val[j][1]; o[3 * j + 2] = val[j][2]; }
      } else {
#pragma unroll
        for (int j = 0; j < kTabPer; ++j)
          if (i0 + j + 1 < L) { o[3 * j] = val[j][0]; o[3 * j + 1] = val[j][1]; o[3 * j + 2] = val[j][2]; }
      }
    }
  }
}

typedef unsigned int ed_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int ed_v2u __attribute__((ext_vector_type(2)));

// Emissions from the tables.  A workgroup owns a tile of (4 * 64 / TW) exons x TW samples; a wave covers 64 / TW exon rows of
// it, lane = (row, sample).  TW is what an XCD's L2 must hold the tables of (the workgroup numbering deals XCD x the sample
// blocks x, x + 8, ... ONE at a time, as k_emit_batch does): 16 samples x ~0.3 MB of hot entries.  Counts and likelihood
// rows are streamed with nontemporal hints so that they do not evict the tables.  Same segment / launch-range interface as
// k_emit_batch (seg built for this tile shape: ed_batch::seg_t).  Launched with TW = kTabTw.
template <int TW>
__global__ void __launch_bounds__(kTabBlock)
k_emit_tab(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const int4* __restrict__ dims,
           const double* __restrict__ tabs, int64_t stride, const int64_t* __restrict__ seg, int nseg, int64_t blk_base,
           int64_t S, uint32_t nsb, double* __restrict__ loglik, uint2* __restrict__ cold_list, unsigned int* __restrict__ cold_n,
           unsigned int cold_cap)
{
  constexpr int RW = 64 / TW;            // exon rows per wave
  constexpr int kRows = 4 * RW;          // ... per workgroup
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t blk = (int64_t)blockIdx.x + blk_base;
  int si;
  int64_t seg_first, seg_e0, e_end;
  {
    const bool has = lane < nseg;
    const int64_t f = has ? seg[3 * lane] : 0, a = has ? seg[3 * lane + 1] : 0, z = has ? seg[3 * lane + 2] : 0;
    si = __popcll(ed_ballot(has && f <= blk)) - 1;
    if (nseg > 64) while (si + 1 < nseg && seg[3 * (si + 1)] <= blk) ++si;
    if (si < 64) {
      auto pick = [&](int64_t v) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, si);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), si);
        return (int64_t)(((uint64_t)hi << 32) | lo);
      };
      seg_first = pick(f); seg_e0 = pick(a); e_end = pick(z);
    } else {
      seg_first = seg[3 * si]; seg_e0 = seg[3 * si + 1]; e_end = seg[3 * si + 2];
    }
  }
  const uint32_t local = (uint32_t)(blk - seg_first);
  uint32_t eb, sb;
  if (nsb >= 8) {
    const uint32_t nsg = (nsb + 7) / 8, per_super = kTabRun * 8 * nsg;
    const uint32_t sup = local / per_super, idx = local - sup * per_super;
    const uint32_t r = idx / (kTabRun * 8), rem = idx % (kTabRun * 8);
    eb = sup * kTabRun + rem / 8;
    sb = (rem % 8) + 8 * r;
    if (sb >= nsb || seg_e0 + (int64_t)eb * kRows >= e_end) return;
  } else {
    eb = local / nsb;
    sb = local - eb * nsb;
  }
  const int wrow = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t e_w0 = seg_e0 + (int64_t)eb * kRows + (int64_t)wrow * RW;     // the wave's first exon row (scalar)
  if (e_w0 >= e_end) return;
  const int64_t s0 = (int64_t)sb * TW;
  const int srel = lane % TW, rrel = lane / TW;
  const int64_t e = e_w0 + rrel;
  const bool live = e < e_end && s0 + srel < S;
  const uint32_t kOOB = 0x7fffffffu;
  // counts: one resource from the wave's first row; lanes that are not live read beyond it (zeros)
  const int32_t cbytes = (int32_t)(((int64_t)(RW - 1) * S + TW) * 4);
  const uint32_t coff = live ? (uint32_t)(((int64_t)rrel * S + srel) * 4) : kOOB;
  const int32_t obs = __builtin_amdgcn_raw_buffer_load_b32(ed_rsrc(test + (e_w0 * S + s0), cbytes), coff, 0, 2);
  const int32_t nref = __builtin_amdgcn_raw_buffer_load_b32(ed_rsrc(ref + (e_w0 * S + s0), cbytes), coff, 0, 2);
  const ed_v4u dq = __builtin_amdgcn_raw_buffer_load_b128(ed_rsrc(dims + s0, TW * 16), live ? (uint32_t)srel * 16u : kOOB, 0, 0);
  const int Ly = (int)dq.x, Lr = (int)dq.y;
  const bool intab = live && tab_cell_served(obs, nref, Ly, Lr, (int)dq.z, (int)dq.w);
  const bool cold = live && !intab && Ly != 0;      // (a sample without tables is walked whole by k_tab_cold: no list entries)
  // the tile's tables: TW samples, `stride` entries of 24 bytes apart (TW * stride * 24 < 2^31: ed_batch_set_emit_mode)
  const __amdgpu_buffer_rsrc_t rt = ed_rsrc(tabs + s0 * stride * 3, (int32_t)((int64_t)TW * stride * 24));
  const uint32_t sbase = (uint32_t)srel * (uint32_t)stride;
  const uint32_t o1 = intab ? (sbase + (uint32_t)obs) * 24u : kOOB;
  const uint32_t o2 = intab ? (sbase + (uint32_t)(Ly + nref)) * 24u : kOOB;
  const uint32_t o3 = intab ? (sbase + (uint32_t)(Ly + Lr + obs + nref)) * 24u : kOOB;
  const ed_v4u a1 = __builtin_amdgcn_raw_buffer_load_b128(rt, o1, 0, 0);
  const ed_v2u b1 = __builtin_amdgcn_raw_buffer_load_b64(rt, o1 + 16u, 0, 0);
  const ed_v4u a2 = __builtin_amdgcn_raw_buffer_load_b128(rt, o2, 0, 0);
  const ed_v2u b2 = __builtin_amdgcn_raw_buffer_load_b64(rt, o2 + 16u, 0, 0);
  const ed_v4u a3 = __builtin_amdgcn_raw_buffer_load_b128(rt, o3, 0, 0);
  const ed_v2u b3 = __builtin_amdgcn_raw_buffer_load_b64(rt, o3 + 16u, 0, 0);
  // cells outside their sample's tables: one atomic per wave
  {
    const unsigned long long m = ed_ballot(cold);
    if (m != 0ull) {
      const unsigned int li = ((unsigned int)blockIdx.x * 4u + (unsigned int)wrow) % (unsigned int)kColdLists, per = cold_cap / kColdLists;
      unsigned int basec = 0;
      if (lane == 0) basec = atomicAdd(cold_n + li, (unsigned int)__popcll(m));
      basec = (unsigned int)__builtin_amdgcn_readfirstlane((int)basec);
      if (cold) {
        const unsigned int at = basec + (unsigned int)ed_rank(m);
        if (at < per) cold_list[(size_t)li * per + at] = make_uint2((unsigned int)e, (unsigned int)(s0 + srel));
        else cold_n[kColdLists] = 1u;
      }
    }
  }
  auto f64 = [](unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); };
  const double v0 = ed_dtab_combine(f64(a1.x, a1.y), f64(a2.x, a2.y), f64(a3.x, a3.y));
  const double v1 = ed_dtab_combine(f64(a1.z, a1.w), f64(a2.z, a2.w), f64(a3.z, a3.w));
  const double v2 = ed_dtab_combine(f64(b1.x, b1.y), f64(b2.x, b2.y), f64(b3.x, b3.y));
  // the rows [e][st][s0 ..]: one resource from the wave's first row, rows S * 8 bytes apart
  const __amdgpu_buffer_rsrc_t rl = ed_rsrc(loglik + (e_w0 * 3 * S + s0), (int32_t)((((int64_t)RW * 3 - 1) * S + TW) * 8));
  const uint32_t loff = intab ? (uint32_t)(((int64_t)rrel * 3 * S + srel) * 8) : kOOB;
  const int32_t rowb = (int32_t)(S * 8);
  ed_buf_store_f64_nt(rl, loff, 0, v0);
  ed_buf_store_f64_nt(rl, loff, rowb, v1);
  ed_buf_store_f64_nt(rl, loff, 2 * rowb, v2);
}

// The cells k_emit_tab left out, through the strict arithmetic: log B(a1 + obs, a2 + tot - obs) - log B(a1, a2) by the
// reference's own routes (edsf::lnbeta; reflection / singular branches and GSL error events included), i.e. the bits
// emit mode 0 writes.  Normally: the lists.  A list ran out (a batch whose samples mostly have no tables): every cell of the
// segments j0 .. j1-1 is looked at again and the ones outside their tables are evaluated.
__device__ __forceinline__ int tab_cold_cell(const int32_t* __restrict__ test, const int32_t* __restrict__ ref,
                                             const double* __restrict__ consts, const int* __restrict__ cflags, int64_t S, int64_t e,
                                             int64_t s, double* __restrict__ loglik, int64_t le, int64_t lst, int64_t ls, int64_t ce, int64_t cs, int cb)
{
  const int32_t obs = ed_ldc(test, e * ce + s * cs, cb);          // count of (e, s): (ce, cs) = (S, 1) for [E][S], (1, E) for [S][E]
  const int32_t tot = obs + ed_ldc(ref, e * ce + s * cs, cb);
  const bool empty = (obs | tot) == 0;
  int nflag = (cflags[s] + cflags[S + s] + cflags[2 * S + s]) * (empty ? 2 : 1);
#pragma unroll 1
  for (int st = 0; st < 3; ++st) {
    const double c = consts[(st * 3 + 2) * S + s];
    double v = c;                                   // a cell without reads: the reference's second call repeats the first
    if (!empty) {
      int flag = 0;
      v = edsf::lnbeta(consts[(st * 3 + 0) * S + s] + (double)obs, (consts[(st * 3 + 1) * S + s] + (double)tot) - (double)obs, &flag);
      nflag += flag;
    }
    loglik[e * le + st * lst + s * ls] = v - c;     // (e, st, s) of [E][3][S] (le, lst, ls = 3 S, S, 1) or of [S][3][Epad] (1, Epad, 3 Epad)
  }
  return nflag;
}

// stats (the words of ed_batch::d_nerr behind the error count and k_emit_batch's flag): [0] cells the lists held, summed over the
// run's launch groups; [1] launch groups whose lists ran out (full re-scan); [2] cells of samples without tables; [3] samples without tables
__global__ void __launch_bounds__(256)
k_tab_cold(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const double* __restrict__ consts,
           const int* __restrict__ cflags, const int4* __restrict__ dims, const uint2* __restrict__ cold_list,
           const unsigned int* __restrict__ cold_n, unsigned int cold_cap, const int64_t* __restrict__ seg, int j0, int j1, int64_t S,
           double* __restrict__ loglik, unsigned long long* __restrict__ nerr, int64_t le, int64_t lst, int64_t ls, int64_t ce, int64_t cs,
           const unsigned int* __restrict__ notab, unsigned long long* __restrict__ stats, int cb)
{
  int nflag = 0;
  const bool smaj = cs != 1;            // counts [S][E]: walk a sample's exons with consecutive threads
  const bool over = cold_n[kColdLists] != 0u;
  if (!over) {
    const unsigned int per = cold_cap / kColdLists;
    for (unsigned int li = blockIdx.x; li < (unsigned int)kColdLists; li += gridDim.x) {
      const unsigned int n = cold_n[li];
      for (unsigned int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint2 c = cold_list[(size_t)li * per + i];
        nflag += tab_cold_cell(test, ref, consts, cflags, S, (int64_t)c.x, (int64_t)c.y, loglik, le, lst, ls, ce, cs, cb);
      }
    }
  } else {
    for (int j = j0; j < j1; ++j) {
      const int64_t e0 = seg[3 * j + 1], e1 = seg[3 * j + 2];
      const int64_t ne = e1 - e0, ncell = ne * S;
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncell; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = smaj ? e0 + i % ne : e0 + i / S, s = smaj ? i / ne : i % S;
        const int4 d = dims[s];
        if (d.x == 0) continue;          // a sample without tables: the pass below
        if (tab_cell_served(ed_ldc(test, e * ce + s * cs, cb), ed_ldc(ref, e * ce + s * cs, cb), d.x, d.y, d.z, d.w)) continue;
        nflag += tab_cold_cell(test, ref, consts, cflags, S, e, s, loglik, le, lst, ls, ce, cs, cb);
      }
    }
  }
  // samples without tables, whole: kStrictChunks workgroup-sized shares per (sample, segment), dealt over the launch
  const unsigned int nnt = notab[0];
  unsigned long long ntl = 0;
  if (nnt != 0u) {
    constexpr int kStrictChunks = 64;
    for (int j = j0; j < j1; ++j) {
      const int64_t e0 = seg[3 * j + 1], e1 = seg[3 * j + 2];
      if (blockIdx.x == 0 && threadIdx.x == 0) ntl += (unsigned long long)(e1 - e0) * nnt;
      for (int64_t w = blockIdx.x; w < (int64_t)nnt * kStrictChunks; w += gridDim.x) {
        const int64_t s = (int64_t)notab[1 + w / kStrictChunks];
        for (int64_t e = e0 + (w % kStrictChunks) * blockDim.x + threadIdx.x; e < e1; e += (int64_t)kStrictChunks * blockDim.x)
          nflag += tab_cold_cell(test, ref, consts, cflags, S, e, s, loglik, le, lst, ls, ce, cs, cb);
      }
    }
  }
  if (nflag) atomicAdd(nerr, (unsigned long long)nflag);
  if (blockIdx.x == 0) {
    __shared__ unsigned long long red[4];
    unsigned long long n = 0;
    for (int i = threadIdx.x; i < kColdLists; i += blockDim.x) n += cold_n[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long all = red[0] + red[1] + red[2] + red[3];
      if (all) atomicAdd(&stats[0], all);
      if (over) atomicAdd(&stats[1], 1ull);
      if (ntl) atomicAdd(&stats[2], ntl);
      stats[3] = nnt;        // (the list's counter itself may be zeroed for the batch's next run before anybody asks)
    }
  }
}

// ---- sample-major form (emit mode 2) ----------------------------------------------------------------------------------
// k_emit_tab is bound by the L1's miss handling: every gather is an L1 miss (a sample's tables are ~0.3 MB of hot lines, the
// L1 32 KB), 3.4 lines per cell at ~300 cycles each with a bounded number in flight per CU = 15 cycles per cell per CU, whatever
// the tile shape (PMC, profiles/r04_*).  The cure is to keep the tables in LDS -- which only one SAMPLE per workgroup can afford:
// 147 KB hold 6 144 entries, the hot 85-99 % of a sample's three tables.  So this form walks the data sample-major:
//   counts    int32 [S][E]            (R's own column-major E x S matrix; made from the [E][S] inputs by k_rows_to_cols for now)
//   loglik    f64   [S][3][Epad]      (k_viterbi_sm reads it through LDS transposition; the [E][3][S] form is made on request)
// A workgroup (16 waves) owns one sample and a share of the launch's 64-exon blocks; a wave reads 64 consecutive exons
// (256 B per matrix), looks its three entries up in LDS (or, beyond the LDS range, in the global tables: L2) and writes three
// 512-byte rows.  Workgroup i runs on XCD i % 8: the shares of one sample sit on one XCD.  Counts are loaded and likelihoods
// stored nontemporally.
// Round 4, what bounds this kernel (1.9 ms per 200 000 x 1024 launch, 3.5 TB/s of its 33 B/cell), from timing builds that each left
// one part out: without its stores 1.27 ms, without its LDS look-ups 1.94 (no change), without the look-ups in the
// global tables 1.72.  So: not the LDS; the stores cost 0.66 ms; and the read side alone is slow -- a wave has one block of counts
// (512 B) in flight, 8 KB per CU, ~1 TB/s at the loaded latency, and cannot have more: the vector-memory counter completes in order
// and the loop holds operations that may or may not be issued (masked global look-ups, masked stores, the list's atomic), so before
// a use the compiler can only rely on what is certainly behind the awaited load and every wait drains the queue (a 3-blocks-ahead
// ring of counts: same 1.9 ms).  Two rewrites with an unconditional, fixed-order loop (256 exons per wave and turn, waits of
// vmcnt(12) / vmcnt(20) in the ISA) were built and measured: with the non-resident cells left to a second kernel the streaming kernel
// ran at 1.50 ms, but patching the warm cells afterwards is 3.6 x 10^7 scattered 8-byte stores = partial-line read-modify-writes,
// 3.0 ms; with the warm cells' entries fetched one cell per lane by lanes 0 .. n-1 and handed back through ds_bpermute before the
// row stores: 1.89 ms -- the exposed round trip to the L2 per turn costs what the pipeline gained; and with every request given a
// whole turn to complete (counts two turns ahead, the warm cells' masked look-ups issued one turn ahead, unrolled by two so that
// no register holding a pending load is moved; waits of vmcnt(6..9) only): 1.78 ms -- the masked gathers themselves, executed by
// nearly every wave and turn for the 10 % of the cells that are warm (ref or tot >= 2 476; 3 % at a window of 4 000 entries, which
// the LDS cannot hold), cost what the pipeline gains.  None is kept: the look-ups beyond the resident windows are what this
// kernel's time is made of once the stores are paid, and only tables that fit (shallower data, or smaller entries) remove them.
constexpr int kSmBlock = 1024;   // 16 waves: 8- and 12-wave workgroups were slower (profiles/r05_ab_sm_threads.txt)

// A tail sample's share of a launch (see tab_windows above): the same walk as the table samples', but an index beyond its LDS window is served by
// Stirling's series instead of a look-up in global memory -- no tables exist there -- and cells count as served up to the conditioning limit.  The
// sample's windows (back to back in global memory), the logarithm's table and the nine (shape parameter, log Gamma of it) triples sit in LDS.  Called
// by k_emit_tab_sm for the workgroups whose sample is a tail sample: ONE launch serves both kinds (a kernel of its own for the tail samples -- 150 KB
// of LDS per workgroup, i.e. a CU to itself -- trickled through the chip behind the other lanes' emission launches even when it had nothing to do:
// 1.8 ms per launch in the headline's kernel trace, profiles/r06_c; the registers of the two loops do not add up, and 128 of them keep the 16 waves).
template <int cb>
__device__ __forceinline__ void emit_tail_share(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const int4 d, const int4 w,
                                                const double* __restrict__ lg0, const double* __restrict__ consts, const double* __restrict__ T,
                                                const int2* __restrict__ blkmap, int64_t nblk_all, int64_t b_begin, int64_t b_end, int64_t S, int64_t E,
                                                int64_t s, int64_t Epad, double* __restrict__ lrow, uint2* __restrict__ cold_list, unsigned int* __restrict__ cold_n,
                                                unsigned int cold_cap, double* __restrict__ lds, double* __restrict__ s_logt, double* __restrict__ s_par)
{
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int64_t kStep = kSmBlock / 64;
  const unsigned int cl = ((unsigned int)blockIdx.x * (unsigned int)(kSmBlock / 64) + (unsigned int)wave) % (unsigned int)kColdLists, cper = cold_cap / kColdLists;
  const int Ly = d.x, Lr = d.y, Tm1 = d.z, N0 = d.w;
  const int n1 = w.x, n2 = w.y, n3 = w.z;
  for (int i = tid; i < ED_PM_LOGT_N * 3; i += kSmBlock) s_logt[i] = (&k_logt_rows[0][0])[i];
  for (int i = tid; i < (n1 + n2 + n3) * 3; i += kSmBlock) lds[i] = T[i];          // the three windows sit back to back (k_tab_build)
  if (tid < 9) {
    const int t = tid / 3, st = tid % 3;
    const double a1 = consts[(st * 3 + 0) * S + s], a2 = consts[(st * 3 + 1) * S + s];
    s_par[tid * 3] = (t == 0) ? a1 : ((t == 1) ? a2 : a1 + a2);                    // (as k_tab_build forms them)
    s_par[tid * 3 + 1] = lg0[((s * 3 + t) * 3 + st) * 2];
    s_par[tid * 3 + 2] = lg0[((s * 3 + t) * 3 + st) * 2 + 1];
  }
  __syncthreads();
  const int64_t row0 = s * E;
  auto ldc = [test, ref, row0](bool is_ref, int64_t e) {
    const int32_t* base = is_ref ? ref : test;
    if (cb == 2) return (int32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(base) + row0 + e);
    return __builtin_nontemporal_load(base + row0 + e);
  };
  auto locate = [&](int64_t bb, int64_t& e, bool& live) {
    const int2 be = blkmap[bb < nblk_all ? bb : nblk_all - 1];
    e = (int64_t)be.x + lane;
    live = bb < b_end && e < (int64_t)be.y;
    if (!live) e = be.x;
  };
  const int nres[3] = {n1, n2, n3}, lbase[3] = {0, n1, n1 + n2};
  int64_t e_n;
  bool live_n;
  locate(b_begin + wave, e_n, live_n);
  int32_t obs_n = ldc(false, e_n), ref_n = ldc(true, e_n);
  for (int64_t b = b_begin + wave; b < b_end; b += kStep) {
    const int64_t e_c = e_n;
    const bool live_c = live_n;
    const int32_t obs = obs_n, nref = ref_n;
    locate(b + kStep, e_n, live_n);                  // the next block's counts are on their way while this one is worked out
    obs_n = ldc(false, e_n);
    ref_n = ldc(true, e_n);
    const bool served = live_c && tab_cell_served(obs, nref, Ly, Lr, Tm1, N0);
    const int idx[3] = {obs, nref, obs + nref};
    double v[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const bool inl = served && idx[t] < nres[t];
      const int li = inl ? (lbase[t] + idx[t]) * 3 : 0;
      v[t][0] = lds[li]; v[t][1] = lds[li + 1]; v[t][2] = lds[li + 2];
      const bool tl = served && !inl;
      if (ed_ballot(tl) != 0ull) {
        if (tl) {
          const double k = (double)idx[t];
#pragma unroll
          for (int st = 0; st < 3; ++st) {
            const double* par = s_par + (t * 3 + st) * 3;
            v[t][st] = ed_dtab_tail(par[0], par[1], par[2], k, s_logt);
          }
        }
      }
    }
    const bool cold = live_c && !served;
    const unsigned long long m = ed_ballot(cold);
    if (m != 0ull) {
      unsigned int basec = 0;
      if (lane == 0) basec = atomicAdd(cold_n + cl, (unsigned int)__popcll(m));
      basec = (unsigned int)__builtin_amdgcn_readfirstlane((int)basec);
      if (cold) {
        const unsigned int at = basec + (unsigned int)ed_rank(m);
        if (at < cper) cold_list[(size_t)cl * cper + at] = make_uint2((unsigned int)e_c, (unsigned int)s);
        else cold_n[kColdLists] = 1u;
      }
    }
    if (served) {
#pragma unroll
      for (int st = 0; st < 3; ++st) __builtin_nontemporal_store(ed_dtab_combine(v[0][st], v[1][st], v[2][st]), lrow + (int64_t)st * Epad + e_c);
    }
  }
}

template <int cb>       // bytes per count, a compile-time constant here: as a run-time argument the 16-bit form of this loop ran at 2.1 ms per launch against 1.8
__global__ void __launch_bounds__(kSmBlock)
k_emit_tab_sm(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const int4* __restrict__ dims,
              const double* __restrict__ tabs, int64_t stride, const int2* __restrict__ blkmap, int64_t nblk_all, int64_t blk0, int64_t nblk,
              int nsplit, int64_t S, int64_t E, int64_t Epad, double* __restrict__ loglik, uint2* __restrict__ cold_list,
              unsigned int* __restrict__ cold_n, unsigned int cold_cap, const int4* __restrict__ wins, const double* __restrict__ lg0,
              const double* __restrict__ consts)
{
  __shared__ double lds[kSmEntries * 3];
  __shared__ double s_logt[ED_PM_LOGT_N * 3];      // (tail samples only: the logarithm's table and the series' per-sample constants)
  __shared__ double s_par[27];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t k = blockIdx.x >> 3;
  const int64_t s = (k / nsplit) * 8 + (blockIdx.x & 7);
  const int chunk = (int)(k % nsplit);
  if (s >= S) return;
  const int4 d = dims[s];
  const int Ly = d.x, Lr = d.y, Ln = Ly + Lr, Tm1 = d.z, N0 = d.w;
  if (Ly == 0) return;             // a sample without tables: k_tab_cold walks it whole (no list entries)
  const int4 wn = wins[s];
  if (wn.w) {                      // a tail sample: Stirling's series beyond the windows
    const int64_t per_t = (nblk + nsplit - 1) / nsplit;
    const int64_t tb0 = blk0 + (int64_t)chunk * per_t;
    const int64_t tb1 = (tb0 + per_t < blk0 + nblk) ? tb0 + per_t : blk0 + nblk;
    emit_tail_share<cb>(test, ref, d, wn, lg0, consts, tabs + s * stride * 3, blkmap, nblk_all, tb0, tb1, S, E, s, Epad, loglik + s * 3 * Epad, cold_list, cold_n,
                        cold_cap, lds, s_logt, s_par);
    return;
  }
  // (Round 5: the entries dealt in proportion to the tables' lengths -- "the same share of every table", the obs table no longer whole in LDS -- were
  //  measured: the launch alone 2.01 against 1.85 ms, the step 4.41 against 4.25.  A cell's three indices do not move together closely enough: the obs count
  //  carries the beta-binomial noise on top of the exon's depth, so a shortened obs window adds warm cells of its own.  profiles/r05_ab_sm_split.txt)
  const int n1 = Ly < kSmT1Max ? Ly : kSmT1Max;
  int n2 = (kSmEntries - n1) / 2;
  if (n2 > Lr) n2 = Lr;
  int n3 = kSmEntries - n1 - n2;
  if (n3 > Ln) n3 = Ln;
  const double* __restrict__ T = tabs + s * stride * 3;
  // fill: three runs of doubles, coalesced, four loads in flight per thread
  auto fill = [&](int l0, int64_t g0, int n) {
    for (int i = tid; i < n; i += 4 * kSmBlock) {
      double q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = (i + u * kSmBlock < n) ? T[g0 + i + u * kSmBlock] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i + u * kSmBlock < n) lds[l0 + i + u * kSmBlock] = q[u];
    }
  };
  fill(0, 0, n1 * 3);
  fill(n1 * 3, (int64_t)Ly * 3, n2 * 3);
  fill((n1 + n2) * 3, (int64_t)Ln * 3, n3 * 3);
  __syncthreads();
  const int64_t per = (nblk + nsplit - 1) / nsplit;
  const int64_t b_begin = blk0 + (int64_t)chunk * per;
  const int64_t b_end = (b_begin + per < blk0 + nblk) ? b_begin + per : blk0 + nblk;
  double* __restrict__ lrow = loglik + s * 3 * Epad;
  // A three-stage software pipeline over the wave's blocks, one block per stage: (A) the counts of block i + 1 are requested;
  // (B) block i's entries are looked up in LDS and, for the lanes whose index lies beyond the resident part, requested from the
  // global tables (every lane loads -- entry 0 where it needs nothing: one address, a broadcast -- so there is no branch);
  // (C) block i - 1's values are combined and stored.  The vector-memory counter completes in order, so a wave that waited for
  // its global lookups right away would also wait for the counts it had just requested: HBM latency once per block with 16
  // waves per CU to hide it.  Where a block's exons are comes from a per-block map read with SCALAR loads (the block number is
  // wave-uniform): nothing in the loop drains the vector-memory queue.
  constexpr int64_t kStep = kSmBlock / 64;
  auto locate = [&](int64_t bb, int64_t& e, bool& live) {
    const int2 be = blkmap[bb < nblk_all ? bb : nblk_all - 1];     // (first exon of the block, its end)
    e = (int64_t)be.x + lane;
    live = bb < b_end && e < (int64_t)be.y;
    if (!live) e = be.x;            // a valid address; nothing is stored for it
  };
  const unsigned int cl = ((unsigned int)blockIdx.x * (unsigned int)(kSmBlock / 64) + (unsigned int)wave) % (unsigned int)kColdLists, cper = cold_cap / kColdLists;
  const int nres[3] = {n1, n2, n3}, lbase[3] = {0, n1, n1 + n2};
  const int64_t gbase[3] = {0, (int64_t)Ly, (int64_t)Ln};
  int64_t e_n;
  bool live_n;
  locate(b_begin + wave, e_n, live_n);
  // (round 5's timing build read the counts "as if 16 bits wide" to price a 16-bit device format: profiles/r05_u16_experiment.txt; cb = 2 is that format)
  const int64_t row0 = s * E;
  auto ldc = [test, ref, row0](bool is_ref, int64_t e) {
    const int32_t* base = is_ref ? ref : test;
    if (cb == 2) return (int32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(base) + row0 + e);
    return __builtin_nontemporal_load(base + row0 + e);
  };
  int32_t obs_n = ldc(false, e_n), ref_n = ldc(true, e_n);
  // stage C's operands
  double v_p[3][3], g_p[3][3];
  bool outl_p[3] = {false, false, false}, intab_p = false, live_p = false;
  int64_t e_p = 0;
  bool have_prev = false;
  for (int64_t b = b_begin + wave;; b += kStep) {
    const bool cur = b < b_end;                       // wave-uniform
    double v_c[3][3], g_c[3][3];
    bool outl_c[3] = {false, false, false}, intab_c = false, live_c = false;
    int64_t e_c = 0;
    if (cur) {
      e_c = e_n; live_c = live_n;
      const int32_t obs = obs_n, nref = ref_n;
      intab_c = live_c && tab_cell_served(obs, nref, Ly, Lr, Tm1, N0);
      const int idx[3] = {obs, nref, obs + nref};
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const bool inl = intab_c && idx[t] < nres[t];
        const int li = inl ? (lbase[t] + idx[t]) * 3 : 0;
        v_c[t][0] = lds[li]; v_c[t][1] = lds[li + 1]; v_c[t][2] = lds[li + 2];
        outl_c[t] = intab_c && !inl;
        g_c[t][0] = g_c[t][1] = g_c[t][2] = 0.0;
        if (outl_c[t]) {     // only the lanes that need it: the texture addresser's time goes with the active lanes
          const double* q = T + (gbase[t] + idx[t]) * 3;
          g_c[t][0] = q[0]; g_c[t][1] = q[1]; g_c[t][2] = q[2];
        }
      }
      locate(b + kStep, e_n, live_n);
      obs_n = ldc(false, e_n);
      ref_n = ldc(true, e_n);
    }
    if (have_prev) {
      const bool cold = live_p && !intab_p;
      const unsigned long long m = ed_ballot(cold);
      if (m != 0ull) {
        unsigned int basec = 0;
        if (lane == 0) basec = atomicAdd(cold_n + cl, (unsigned int)__popcll(m));
        basec = (unsigned int)__builtin_amdgcn_readfirstlane((int)basec);
        if (cold) {
          const unsigned int at = basec + (unsigned int)ed_rank(m);
          if (at < cper) cold_list[(size_t)cl * cper + at] = make_uint2((unsigned int)e_p, (unsigned int)s);
          else cold_n[kColdLists] = 1u;
        }
      }
      if (intab_p) {
#pragma unroll
        for (int st = 0; st < 3; ++st) {
          const double d1 = outl_p[0] ? g_p[0][st] : v_p[0][st], d2 = outl_p[1] ? g_p[1][st] : v_p[1][st], d3 = outl_p[2] ? g_p[2][st] : v_p[2][st];
          __builtin_nontemporal_store(ed_dtab_combine(d1, d2, d3), lrow + (int64_t)st * Epad + e_p);
        }
      }
    }
    if (!cur) break;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      outl_p[t] = outl_c[t];
#pragma unroll
      for (int st = 0; st < 3; ++st) { v_p[t][st] = v_c[t][st]; g_p[t][st] = g_c[t][st]; }
    }
    intab_p = intab_c; live_p = live_c; e_p = e_c; have_prev = true;
  }
}

// [S][3][Epad] -> [E][3][S]: the documented layout of the likelihood matrix, made on request (accessors, verification)
__global__ void __launch_bounds__(256)
k_ll_sm_to_rows(const double* __restrict__ in, int64_t E, int64_t Epad, int64_t S, double* __restrict__ out)
{
  __shared__ double tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t e0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
  const int st = blockIdx.z;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t s = s0 + ty + 4 * k, e = e0 + tx;
    tile[ty + 4 * k][tx] = (s < S && e < E) ? in[(s * 3 + st) * Epad + e] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t e = e0 + ty + 4 * k, s = s0 + tx;
    if (e < E && s < S) out[(e * 3 + st) * S + s] = tile[tx][ty + 4 * k];
  }
}

// int32 [E][n] -> [n][E] (the sample-major copy of the counts; 64 x 64 tiles through LDS)
__global__ void __launch_bounds__(256)
k_tab_rows_to_cols(const int32_t* __restrict__ in, int64_t E, int64_t n, int32_t* __restrict__ out)
{
  __shared__ int32_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t e0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t e = e0 + ty + 4 * k, s = s0 + tx;
    tile[ty + 4 * k][tx] = (e < E && s < n) ? in[e * n + s] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t s = s0 + ty + 4 * k, e = e0 + tx;
    if (s < n && e < E) out[s * E + e] = tile[tx][ty + 4 * k];
  }
}

// k_viterbi for the sample-major likelihood matrix [S][3][Epad].  Same chain layout (a quad of lanes per chain, lane j = HMM
// state j, 16 chains per wave), same arithmetic and association order, same back-pointer words: only the way the emissions
// reach the register ring differs.  A lane's emissions are now CONTIGUOUS in memory (its chain's row of its state), so one
// 16-byte load per lane would touch 48 different lines per instruction; instead the wave loads a tile of 16 steps for its 48
// rows cooperatively -- lane l takes 16 bytes (2 steps) of row 8 k + l / 8, k = 0..5: eight whole 128-byte lines per
// instruction -- parks it in LDS (rows 144 bytes apart: 16-byte reads by 48 rows spread over all banks) and every lane reads
// its own row back, two steps per ds_read_b128, as the ring slots are consumed.  Tile T + 3 is in flight from memory while
// tile T + 2 is read from LDS and tiles T, T + 1 are in registers.  Loads run past the chromosome's end (into the next
// chromosome's emissions or the next row; the matrix is padded): what is loaded there is never used.
// Work distribution.  queue == nullptr: workgroup (x, y) = (sample group x, job job_base + y), as k_viterbi.  queue != nullptr (what
// ed_batch_run launches): a PERSISTENT grid of `gridDim.x` waves -- one per SIMD of the chip -- pulls (job, sample group) items from
// a counter, all groups of the longest chromosome first (the jobs are sorted by decreasing length: dynamic longest-processing-time).
// Why (round 5 trace, profiles/r05_timeline_*.txt): a step of the recurrence is ~27 dependent wave64 instructions = ~110 cycles of ONE
// SIMD's issue port whether one or two waves live on it, so 24 x 64 = 1 536 one-chromosome waves on 1 024 SIMDs finish when the 512
// SIMDs holding two of them do, and for as long as they run every SIMD holding two (2 x 251 registers) is closed to any other
// kernel: the next slab's table build and fit, queued beside them, waited ~0.6 ms for the first chains to retire.  With one wave per
// SIMD the makespan is the longest chromosome's chain (it cannot be less) and 261 registers per SIMD stay free for the neighbours.
// queue[0]: next item; queue[1]: waves that have left -- the last one zeroes both for the next launch.
__global__ void __launch_bounds__(kWave, 1)
k_viterbi_sm(const double* __restrict__ loglik, int64_t Epad, const double* __restrict__ lt4, double c0, double c1,
             const int32_t* __restrict__ chrom_off, const int64_t* __restrict__ word_off, int64_t S, int32_t C,
             uint32_t* __restrict__ bpq, uint8_t* __restrict__ last, const int32_t* __restrict__ job_off,
             const int32_t* __restrict__ job_chrom, int job_base, unsigned int* __restrict__ queue, unsigned int n_groups, unsigned int n_items)
{
  const int lane = threadIdx.x;
  const int j = lane & 3;
  __shared__ double2 lds_lt[2][kVitTile][4];
  constexpr int kRowD = 18;                                   // doubles between rows in LDS (144 bytes)
  __shared__ __attribute__((aligned(16))) double lds_em[2][48 * kRowD];
  // The recurrence is one dependent chain per wave and the longest chromosome's chain IS the launch's makespan: a wave of another kernel
  // on the same SIMD (the next slab's table build and fit run beside this launch) that takes every other issue slot doubles it.  With a
  // raised priority the chain issues whenever it can and the neighbours get the slots its dependencies leave empty.
  __builtin_amdgcn_s_setprio(3);
  for (;;) {
  unsigned int item = 0;
  if (queue) {
    if (lane == 0) item = atomicAdd(queue, 1u);
    item = (unsigned int)__builtin_amdgcn_readfirstlane((int)item);
    if (item >= n_items) break;
  }
  const int64_t s_first = (int64_t)(queue ? item % n_groups : blockIdx.x) * kVitChains;
  const int64_t s_raw = s_first + (lane >> 2);
  const bool live = s_raw < S;
  const int64_t s = live ? s_raw : S - 1;
  const int job = job_base + (int)(queue ? item / n_groups : blockIdx.y);
  // cooperative loads: row r = 8 k + (lane >> 3) of the wave's 48 (chain r / 3, likelihood column r % 3), piece lane & 7
  uint32_t roff[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int r = 8 * k + (lane >> 3);
    int64_t sr = s_first + r / 3;
    if (sr >= S) sr = S - 1;
    roff[k] = (uint32_t)((((sr - s_first) * 3 + (r % 3)) * Epad) * 8 + (lane & 7) * 16);   // bytes from the wave's first row
  }
  const int col = (j == 1) ? 0 : ((j == 2) ? 2 : 1);
  const int myrow = (lane >> 2) * 3 + col;
  for (int jc = job_off[job]; jc < job_off[job + 1]; ++jc) {
  const int c = job_chrom[jc];
  const int64_t lo = chrom_off[c], hi = chrom_off[c + 1];
  const int64_t m = hi - lo;
  if (m <= 0) continue;
  __syncthreads();
  const double2* __restrict__ ltp = reinterpret_cast<const double2*>(lt4) + (lo + c) * 4 + j;
  const int64_t wstride = S * 4;
  const double t0 = (j == 0 || j == 3) ? c0 : c1;
  double v = (j == 0 || j == 3) ? 0.0 : -HUGE_VAL;
  char* __restrict__ bpb = reinterpret_cast<char*>(bpq + word_off[c] * S * 4);
  const uint32_t boff = (uint32_t)((s * 4 + j) * 4);
  const int64_t wbytes = wstride * 4;
  const double2* __restrict__ ltw = reinterpret_cast<const double2*>(lt4) + (lo + c) * 4;
  const int m32 = (int)m;
  const char* __restrict__ embase = reinterpret_cast<const char*>(loglik + (s_first * 3 * Epad + lo));   // wave-uniform
  typedef double v2d __attribute__((ext_vector_type(2)));
  typedef double v2d_a8 __attribute__((ext_vector_type(2), aligned(8)));     // a chromosome may start at an odd exon: 8-byte aligned rows
  auto coop = [&](int T, v2d (&g)[6]) {
    const char* tb = embase + (int64_t)T * (kVitTile * 8);
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = *reinterpret_cast<const v2d_a8*>(tb + roff[k]);
  };
  auto park = [&](int buf, const v2d (&g)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      *reinterpret_cast<v2d*>(&lds_em[buf][(8 * k + (lane >> 3)) * kRowD + (lane & 7) * 2]) = g[k];
  };
  constexpr int kRing = 2 * kVitTile;
  double er[kRing];
  // staging registers of the cooperative loads: two sets in rotation.  Tile t + 4 is requested at the top of tile t and parked at the
  // end of tile t + 1: two tiles of cover.  (With one set, tile t + 3 was requested at the top of tile t and parked at its end -- 16
  // steps = ~0.8 us later, less than a loaded HBM round trip, and with ONE wave per SIMD (the persistent grid) nobody else issues
  // while it waits: profiles/r05_ab_vitdepth.txt.)
  v2d stgs[2][6];
  double2 stl = ltw[lane];
  // prologue: tiles 0 and 1 into the ring, tile 2 into LDS buffer 0, tiles 3 and 4 in flight at the top of tile 0
  v2d (&stg)[6] = stgs[0];
  coop(0, stg); park(0, stg);
  coop(1, stg); park(1, stg);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kVitTile / 2; ++q) {
    const v2d a = *reinterpret_cast<const v2d*>(&lds_em[0][myrow * kRowD + 2 * q]);
    const v2d b = *reinterpret_cast<const v2d*>(&lds_em[1][myrow * kRowD + 2 * q]);
    er[2 * q] = a.x; er[2 * q + 1] = a.y;
    er[kVitTile + 2 * q] = b.x; er[kVitTile + 2 * q + 1] = b.y;
  }
  coop(2, stg);
  (&lds_lt[0][0][0])[lane] = stl;
  __syncthreads();
  park(0, stg);
  coop(3, stgs[1]);
  auto tile = [&](auto par, int t, int nsteps, bool full) {
    constexpr int P = decltype(par)::value;
    stl = ltw[(t + 1) * 64 + lane];
    coop(t + 4, stgs[P]);
    uint32_t w = 0;
#pragma unroll
    for (int g4 = 0; g4 < kVitTile / 4; ++g4) {
      double2 lrow[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) lrow[k] = lds_lt[P][g4 * 4 + k][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kk = g4 * 4 + k;
        if (full || kk < nsteps) {
          unsigned fw = vit_step_q(v, er[P * kVitTile + kk], t0, lrow[k].x, lrow[k].y);
          asm("" : "+v"(fw));
          w |= fw << (2 * kk);
        }
        if (kk & 1) {     // the two slots just consumed take steps kk - 1, kk of tile t + 2 (LDS buffer P)
          const v2d nx = *reinterpret_cast<const v2d*>(&lds_em[P][myrow * kRowD + (kk - 1)]);
          er[P * kVitTile + kk - 1] = nx.x; er[P * kVitTile + kk] = nx.y;
        }
      }
    }
    *reinterpret_cast<uint32_t*>(bpb + (int64_t)t * wbytes + boff) = w;
    (&lds_lt[P ^ 1][0][0])[lane] = stl;
    park(P ^ 1, stgs[P ^ 1]);   // tile t + 3 -> the buffer tile t + 1 was read from during tile t - 1
    __syncthreads();
  };
  {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const int ntile = (m32 + kVitTile - 1) / kVitTile;
    const int nfull = (m32 / kVitTile) & ~1;
    int t = 0;
    for (; t < nfull; t += 2) {
      tile(I0{}, t, kVitTile, true);
      tile(I1{}, t + 1, kVitTile, true);
    }
    for (; t < ntile; ++t) {
      const int nst = (m32 - t * kVitTile < kVitTile) ? (m32 - t * kVitTile) : kVitTile;
      if (t & 1) tile(I1{}, t, nst, false);
      else tile(I0{}, t, nst, false);
    }
  }
  int st;
  {
    const double2 l = ltp[m * 4];
    const double e = (j == 1) ? 0.0 : -100.0;
    const unsigned fw = vit_step_q(v, e, t0, l.x, l.y);
    st = quad_bcast_i<0>((int)fw);
  }
  if (live && j == 0) last[(int64_t)c * S + s] = (uint8_t)st;
  }
  if (!queue) break;
  }
  if (queue && lane == 0) {
    if (atomicAdd(queue + 1, 1u) == gridDim.x - 1u) { queue[0] = 0u; queue[1] = 0u; }     // (every wave has taken its last item by now)
  }
}

// Tolerance form of the self-check (ed_batch_verify_emissions_tol): every cell evaluated again with the reference's own
// per-cell loop, as k_emit_verify does, and compared with the likelihood matrix as  |got - want| <= max(abs_tol, rel_tol |want|)
// (NaN matches NaN, equal infinities match).  counters: [0] values beyond the tolerance, [1] values compared, [2] records
// written to `first`, [3] bits of the largest relative difference seen among finite non-zero `want`, [4] ... absolute.
__global__ void __launch_bounds__(kEmitBlock)
k_emit_verify_tol(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const double* __restrict__ phi,
                  const double* __restrict__ expected, double mixture, int64_t E, int64_t S, const double* __restrict__ loglik,
                  double rel_tol, double abs_tol, unsigned long long* __restrict__ counters, ed_emit_mismatch* __restrict__ first,
                  int64_t cap, int64_t ce, int64_t cs, int cb, const double* __restrict__ mix_s)
{
  const int64_t s_raw = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int64_t e0 = (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * (kEmitBlock / 64) + (threadIdx.x >> 6)) * kVerifyRun;
  const bool live_s = s_raw < S;
  const int64_t s = live_s ? s_raw : 0;
  const double ex = expected[s];
  const double sd = __builtin_sqrt((phi[s] * ex) * (1. - ex));
  double ep[3];
  state_props(ex, mix_s ? mix_s[s] : mixture, ep);
  int bad = 0, ncell = 0;
  double max_rel = 0.0, max_abs = 0.0;
#pragma unroll 1
  for (int st = 0; st < 3; ++st) {
    double a1, a2;
    shape_params(ep[st], sd, a1, a2);
    int f2 = 0;
    const double v0 = edsf::lnbeta(a1, a2, &f2);
#pragma unroll 1
    for (int k = 0; k < kVerifyRun; ++k) {
      const int64_t e = e0 + k;
      const bool live = live_s && e < E;
      const int64_t ec = e < E ? e : E - 1;
      const int32_t obs = ed_ldc(test, ec * ce + s * cs, cb);
      const int32_t tot = obs + ed_ldc(ref, ec * ce + s * cs, cb);
      int f1 = 0;
      const double v1 = edsf::lnbeta(a1 + (double)obs, (a2 + (double)tot) - (double)obs, &f1);
      const double want = v1 - v0;
      const double got = loglik[(ec * 3 + st) * S + s];
      const double diff = fabs(got - want);
      const bool same = (got == want) || (want != want && got != got) || diff <= fmax(abs_tol, rel_tol * fabs(want));
      if (live && st == 0) ++ncell;
      if (live && diff == diff && diff < HUGE_VAL) {
        max_abs = fmax(max_abs, diff);
        if (want != 0.0) max_rel = fmax(max_rel, diff / fabs(want));
      }
      if (live && !same) {
        ++bad;
        const unsigned long long q = atomicAdd(&counters[2], 1ull);
        if ((int64_t)q < cap) {
          ed_emit_mismatch m;
          m.exon = e; m.sample = s; m.state = st; m.observed = obs; m.total = tot; m.pad_ = 0;
          m.got = got; m.want = want;
          first[q] = m;
        }
      }
    }
  }
  int wbad = bad, wcell = ncell;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    wbad += __shfl_xor(wbad, d, 64);
    wcell += __shfl_xor(wcell, d, 64);
    max_rel = fmax(max_rel, __shfl_xor(max_rel, d, 64));
    max_abs = fmax(max_abs, __shfl_xor(max_abs, d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    if (wbad) atomicAdd(&counters[0], (unsigned long long)wbad);
    if (wcell) atomicAdd(&counters[1], 3ull * (unsigned long long)wcell);
    // non-negative doubles order like their bit patterns
    if (max_rel > 0.0) atomicMax(&counters[3], (unsigned long long)__double_as_longlong(max_rel));
    if (max_abs > 0.0) atomicMax(&counters[4], (unsigned long long)__double_as_longlong(max_abs));
  }
}

}  // namespace
