// edfit_hist.inc -- the histogram form of the dispersion fit (k_fit_hist + k_fit_hnewton), included by edfit.inc once
// per GEOMETRY inside its own namespace with ED_HG_KS = samples per workgroup of k_fit_hist = 8, 4, 2: the 147 KB of LDS
// bins are shared by that many samples, so the unit bins reach 1024 / 4096 / 4096 (y / r / n) at 8 samples and two or
// four times as far at 4 or 2 -- deeper data (counts beyond the bins are evaluated cell by cell, which is what made a
// fit at ~400 reads per exon and sample cost 10 ms instead of 1.3).  fit_columns launches, through the Launch struct at the end
// of this file, the geometry the previous fit's depth points to (all three the first time: fitjob::launched_geometries); a device word set from THIS fit's data (k_fit_start: the largest
// per-sample mean total) decides on the device which of the launched ones runs (fit_hist_runs): no host round trip.
constexpr int kHistId = ED_HG_KS;                        // the geometry: 8, 4 or 2 = samples that share 147 KB worth of bins
constexpr int kHistSamples = kHistId;                    // samples per workgroup of k_fit_hist
constexpr int kHistKy = 1024 * 8 / kHistId;              // bins of the test count
constexpr int kHistKr = 4096 * 8 / kHistId;              // bins of the reference count
constexpr int kHistKn = 4096 * 8 / kHistId;              // bins of the total
constexpr int kHistK = kHistKy + kHistKr + kHistKn;
constexpr int kHistBlock = 1024;
constexpr int kHistHalves = 2;                           // workgroups per sample group: each takes half of the rows
constexpr int kHistRows = kHistBlock / kHistSamples;     // rows per sweep of a workgroup
constexpr int kHistGroups = kHistHalves * kHistRows;     // (half, thread row) pairs = overflow regions per sample
constexpr int kHistChunk = 65535;                        // rows between flushes: a 16-bit bin cannot wrap
static_assert((kHistKy % 2) == 0 && (kHistKr % 2) == 0, "two 16-bit bins per LDS word");

// Second level of the histograms, in LDS of k_fit_hnewton: the cells k_fit_hist could not place (a count beyond its
// bins; 3 % of the cells at ~100 reads per exon and sample, 15 % at ~200) were evaluated one by one in every
// iteration -- as costly as all the bins together at 3 %, the whole fit at 15 % (9.4 ms).  A cell lands there
// because n >= kHistKn (then r = n - y > kHistKn - kHistKy when y is in range), so two more ranges of kOv2 unit bins,
// r in [kOv2R0, kOv2R0 + kOv2) and n in [kHistKn, kHistKn + kOv2), built once per launch from the overflow lists,
// take most of them; what is still outside stays a list (compacted in place) and is evaluated per cell.
constexpr int kOv2 = (kHistId == 2) ? 3072 : 5120;   // what the LDS has room for next to the reduction buffers and res_pre
constexpr int kOv2R0 = kHistKr - kHistKy;
constexpr int kOv2Words = (kHistKy + 2 * kOv2) / 2;   // 16-bit bins, two per word: y | r | n
static_assert(kHistKy % 2 == 0 && kOv2 % 2 == 0, "packed pairs");

// Sample-major form (k_fit_hist_sm): a sample's histograms are ONE contiguous row of the global array, [y | r | n | r2 | n2]:
// the three first-level histograms and -- where the LDS has room for them next to the first level (geometries 8 and 4) -- the two
// second-level ranges above, filled by the histogram kernel itself instead of going through the overflow lists (2.9 % of the
// cells at ~100 reads per exon and sample: 6 x 10^6 scattered 4-byte list writes per 1024 samples, 0.75 GB of partial-line
// traffic, all read back and re-binned by the Newton kernel).  A coordinate takes the first level that holds it; a cell goes
// to the list only if one of its coordinates fits neither.
constexpr bool kSm2 = (kHistId != 2);
constexpr int kSmBins = kHistK + (kSm2 ? 2 * kOv2 : 0);
constexpr int kSmChunk = 49152 - 1024;   // rows between two looks at the bins: a bin below kSmHot at the start of a chunk cannot wrap in it (a multiple of 1024: chunks start 16-byte aligned)
constexpr uint32_t kSmHot = 0x4000;
constexpr int kSmCarry = 128;            // bins moved out of LDS before the end (each holds >= kSmHot cells: 3 E / 16384 of them at most)

// LDS bins are 16 bits wide, two per 32-bit word (the LDS atomic adds 1 or 1 << 16): 8 samples fit where 4 did,
// which halves the L2 -> L1 line traffic the kernel is bound by (a workgroup uses 32 B of every 128-B line of a
// count row instead of 16).  A bin cannot wrap because the bins are flushed to the 32-bit global histogram of
// this half every kHistChunk rows.  hist: [kHistHalves][ceil(S / 8) * 2 quads][kHistK][4]: the four samples of a quad
// side by side and the bins of a quad contiguous, which is how k_fit_hnewton walks it (a wave = 4 samples x 16
// consecutive bins = 256 contiguous bytes, re-read every iteration) and lets the flush below write whole lines.
__host__ __device__ __forceinline__ int64_t hist_padded(int64_t S) { return (S + 7) / 8 * 8; }   // whole quads, whatever the geometry
__device__ __forceinline__ int64_t hist_at(int half, int64_t v, int64_t s, int64_t Sp)
{
  return ((int64_t)half * (Sp >> 2) + (s >> 2)) * (kHistK * 4) + v * 4 + (s & 3);
}

__global__ void __launch_bounds__(kHistBlock)
k_fit_hist(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t rs, int64_t E, int64_t S,
           uint32_t* __restrict__ hist, int32_t* __restrict__ ov_y, int32_t* __restrict__ ov_r, int32_t* __restrict__ ovn,
           int64_t cap /* overflow cells per (overflow region, sample) */, const int* __restrict__ depth_max, int launched)
{
  if (!fit_hist_runs(*depth_max, launched, kHistId)) return;   // another geometry's launch serves this batch
  __shared__ uint32_t hsm[kHistSamples * (kHistK / 2)];
  const int tid = threadIdx.x;
  // Workgroups are dealt to the 8 XCDs round-robin, and neighbouring sample groups share every 128-byte line of a
  // count row: neighbours must sit on the SAME XCD (one L2) or each line is fetched several times.  So XCD x
  // (= blockIdx % 8) owns a contiguous range of the (half, sample group) pairs, half-major.
  const int64_t ng = (S + kHistSamples - 1) / kHistSamples, nwg = ng * kHistHalves, per = (nwg + 7) / 8;
  const int64_t lin = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const bool active = (int64_t)(blockIdx.x >> 3) < per && lin < nwg;
  const int half = active ? (int)(lin / ng) : 0;
  const int64_t grp = active ? lin % ng : 0;
  const int j = tid & (kHistSamples - 1);
  const int64_t s = active ? grp * kHistSamples + j : S;
  uint32_t* __restrict__ h = hsm + j * (kHistK / 2);
  const int64_t Sp = hist_padded(S);
  // this half's rows
  const int64_t r0 = (E * half) / kHistHalves, r1 = (E * (half + 1)) / kHistHalves;
  int nov = 0;   // this thread's overflow cells: stored in row order in its own region -- no atomics, and the
                 // order in which k_fit_hnewton adds them up is the same on every run
  const int region = half * kHistRows + tid / kHistSamples;
  const int64_t ovbase = (int64_t)region * cap;
  auto bump = [&](int v) { atomicAdd(&h[v >> 1], 1u << ((v & 1) * 16)); };
  int chunk_no = 0;
  for (int64_t c0 = r0; c0 < r1 || chunk_no == 0; c0 += kHistChunk, ++chunk_no) {
    const int64_t c1 = (c0 + kHistChunk < r1) ? c0 + kHistChunk : r1;
    for (int i = tid; i < kHistSamples * (kHistK / 2); i += kHistBlock) hsm[i] = 0;
    __syncthreads();
    if (s < S) {
      constexpr int kPre = 4;                              // rows in flight per thread (2 and 8 measured in the pipeline: the same step to 0.05 ms)
      int yb[kPre], rb[kPre];
      const int64_t e0 = c0 + tid / kHistSamples;
#pragma unroll
      for (int k = 0; k < kPre; ++k) {
        const int64_t e = e0 + (int64_t)k * kHistRows;
        yb[k] = (e < c1) ? test[e * rs + s] : 0;
        rb[k] = (e < c1) ? ref[e * rs + s] : 0;
      }
      for (int64_t e = e0; e < c1; e += (int64_t)kPre * kHistRows) {
        int yc[kPre], rc[kPre];
#pragma unroll
        for (int k = 0; k < kPre; ++k) { yc[k] = yb[k]; rc[k] = rb[k]; }
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          const int64_t en = e + (int64_t)(kPre + k) * kHistRows;
          yb[k] = (en < c1) ? test[en * rs + s] : 0;
          rb[k] = (en < c1) ? ref[en * rs + s] : 0;
        }
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          if (e + (int64_t)k * kHistRows >= c1) break;
          const int y = yc[k], r = rc[k];
          const int n = y + r;
          if (n <= 0) continue;   // carries no information (and is not counted), as in accumulate_cell
          if ((unsigned)y < (unsigned)kHistKy && (unsigned)r < (unsigned)kHistKr && (unsigned)n < (unsigned)kHistKn) {
            bump(y);
            bump(kHistKy + r);
            bump(kHistKy + kHistKr + n);
          } else {
            if (nov < cap) { ov_y[(ovbase + nov) * S + s] = y; ov_r[(ovbase + nov) * S + s] = r; }
            ++nov;
          }
        }
      }
    }
    __syncthreads();
    // flush: this workgroup owns its (half, samples) slice of the global histogram
    for (int i = tid; i < kHistSamples * kHistK; i += kHistBlock) {
      int v, jj;
      if constexpr (kHistSamples >= 4) {
        const int quad = i / (kHistK * 4), rem = i % (kHistK * 4);   // consecutive i = consecutive words of the slice
        v = rem >> 2; jj = quad * 4 + (rem & 3);
      } else {
        v = i / kHistSamples; jj = i % kHistSamples;                 // half a quad: pairs of words
      }
      const int64_t ss = grp * kHistSamples + jj;
      if (active && ss < S) {
        const uint32_t cnt = (hsm[jj * (kHistK / 2) + (v >> 1)] >> ((v & 1) * 16)) & 0xffffu;
        uint32_t* __restrict__ o = hist + hist_at(half, v, ss, Sp);
        *o = (chunk_no == 0 ? 0u : *o) + cnt;
      }
    }
    __syncthreads();
  }
  if (s < S) ovn[(int64_t)region * S + s] = nov;
}

// The same histograms from SAMPLE-MAJOR counts ([S][E]: R's column-major matrix as it lies in memory): one workgroup per sample
// walks that sample's contiguous counts, so the LDS bins are ONE sample's (18 / 36 / 72 KB by geometry instead of 147 KB: other
// workgroups fit beside it on the CU) and every load is a coalesced 256-byte row piece.  Same outputs as k_fit_hist: the global
// histogram (all counts in half 0, half 1 zero), the overflow lists (thread t is region t; the other regions stay empty; cells in
// exon order inside a region, so the Newton sums add them in the same order on every run).  pitch: ints between consecutive
// samples; by: exon step (subset.for.speed); E: rows to fit (exons 0, by, 2 by, ...).
constexpr int kHsBlock = 256;
static_assert(kHistGroups >= kHsBlock, "a thread per overflow region");
__global__ void __launch_bounds__(kHsBlock)
k_fit_hist_sm(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t pitch, int64_t by, int64_t E, int64_t S,
              uint32_t* __restrict__ hist, int32_t* __restrict__ ov_y, int32_t* __restrict__ ov_r, int32_t* __restrict__ ovn,
              int64_t cap, const int* __restrict__ depth_max, int launched, int cb)
{
  if (!fit_hist_runs(*depth_max, launched, kHistId)) return;
  __shared__ uint32_t h[kSmBins / 2];
  __shared__ uint32_t carry_bin[kSmCarry], carry_cnt[kSmCarry];
  __shared__ int carry_n;
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  // (cb = 2: the matrices hold uint16 counts; trow / rrow are byte-exact row starts either way and every access goes through rd())
  const int32_t* __restrict__ trow = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(test) + s * pitch * cb);
  const int32_t* __restrict__ rrow = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(ref) + s * pitch * cb);
  auto rd = [cb](const int32_t* rowp, int64_t i) -> int { return ed_ldc(rowp, i, cb); };
  uint32_t* __restrict__ row = hist + s * kSmBins;
  // the lists of this form are sample-major too: [S][kHistGroups][cap], thread t fills region t front to back
  int32_t* __restrict__ oy = ov_y + (s * kHistGroups + tid) * cap;
  int32_t* __restrict__ orr = ov_r + (s * kHistGroups + tid) * cap;
  int nov = 0;
  auto bump = [&](int v) { atomicAdd(&h[v >> 1], 1u << ((v & 1) * 16)); };
  for (int i = tid; i < kSmBins / 2; i += kHsBlock) h[i] = 0;
  if (tid == 0) carry_n = 0;
  __syncthreads();
  auto cell = [&](int y, int r) {
    const int n = y + r;
    if (n <= 0) return;              // carries no information (and is not counted), as in accumulate_cell
    int br = -1, bn = -1;
    if ((unsigned)r < (unsigned)kHistKr) br = kHistKy + r;
    else if (kSm2 && (unsigned)(r - kOv2R0) < (unsigned)kOv2) br = kHistK + (r - kOv2R0);
    if ((unsigned)n < (unsigned)kHistKn) bn = kHistKy + kHistKr + n;
    else if (kSm2 && (unsigned)(n - kHistKn) < (unsigned)kOv2) bn = kHistK + kOv2 + (n - kHistKn);
    if ((unsigned)y < (unsigned)kHistKy && br >= 0 && bn >= 0) {
      bump(y);
      bump(br);
      bump(bn);
    } else {
      if (nov < cap) { oy[nov] = y; orr[nov] = r; }
      ++nov;
    }
  };
  // consecutive exons, 16-byte aligned rows: four exons per lane and load (a thread's list then holds its cells in the order it met
  // them -- still the same order on every run)
  const bool vec = cb == 4 && by == 1 && (pitch & 3) == 0 && ((((uintptr_t)test) | ((uintptr_t)ref)) & 15) == 0;
  const bool vec16 = cb == 2 && by == 1 && (pitch & 7) == 0 && ((((uintptr_t)test) | ((uintptr_t)ref)) & 15) == 0;
  for (int64_t c0 = 0; c0 < E; c0 += kSmChunk) {
    const int64_t c1 = (c0 + kSmChunk < E) ? c0 + kSmChunk : E;
    int64_t cs0 = c0;                // where the scalar walk below starts
    if (vec) {
      typedef int v4i __attribute__((ext_vector_type(4)));
      constexpr int kVPre = 2;
      constexpr int64_t kSpan = (int64_t)kHsBlock * 4;
      const int64_t nfull = (c1 - c0) / kSpan;          // whole spans of 1024 exons in this chunk
      v4i yv[kVPre], rv[kVPre];
#pragma unroll
      for (int k = 0; k < kVPre; ++k) {
        const bool in = k < nfull;
        const int64_t e = c0 + (in ? k : 0) * kSpan + tid * 4;
        yv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v4i*>(trow + e)) : v4i{0, 0, 0, 0};
        rv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v4i*>(rrow + e)) : v4i{0, 0, 0, 0};
      }
      for (int64_t b0 = 0; b0 < nfull; b0 += kVPre) {
        v4i yc[kVPre], rc[kVPre];
#pragma unroll
        for (int k = 0; k < kVPre; ++k) { yc[k] = yv[k]; rc[k] = rv[k]; }
#pragma unroll
        for (int k = 0; k < kVPre; ++k) {
          const bool in = b0 + kVPre + k < nfull;
          const int64_t e = c0 + (in ? b0 + kVPre + k : 0) * kSpan + tid * 4;
          yv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v4i*>(trow + e)) : v4i{0, 0, 0, 0};
          rv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v4i*>(rrow + e)) : v4i{0, 0, 0, 0};
        }
#pragma unroll
        for (int k = 0; k < kVPre; ++k) {
          if (b0 + k >= nfull) break;
          cell(yc[k].x, rc[k].x); cell(yc[k].y, rc[k].y); cell(yc[k].z, rc[k].z); cell(yc[k].w, rc[k].w);
        }
      }
      cs0 = c0 + nfull * kSpan;
    }
    if (vec16) {     // the same with eight 16-bit counts per lane and load
      typedef unsigned short v8h __attribute__((ext_vector_type(8)));
      constexpr int kVPre = 2;
      constexpr int64_t kSpan = (int64_t)kHsBlock * 8;
      const int64_t nfull = (c1 - c0) / kSpan;          // whole spans of 2048 exons in this chunk (chunks start at multiples of 1024: 16-byte aligned)
      const unsigned short* __restrict__ th = reinterpret_cast<const unsigned short*>(trow);
      const unsigned short* __restrict__ rh = reinterpret_cast<const unsigned short*>(rrow);
      const v8h zero = {0, 0, 0, 0, 0, 0, 0, 0};
      v8h yv[kVPre], rv[kVPre];
#pragma unroll
      for (int k = 0; k < kVPre; ++k) {
        const bool in = k < nfull;
        const int64_t e = c0 + (in ? k : 0) * kSpan + tid * 8;
        yv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v8h*>(th + e)) : zero;
        rv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v8h*>(rh + e)) : zero;
      }
      for (int64_t b0 = 0; b0 < nfull; b0 += kVPre) {
        v8h yc[kVPre], rc[kVPre];
#pragma unroll
        for (int k = 0; k < kVPre; ++k) { yc[k] = yv[k]; rc[k] = rv[k]; }
#pragma unroll
        for (int k = 0; k < kVPre; ++k) {
          const bool in = b0 + kVPre + k < nfull;
          const int64_t e = c0 + (in ? b0 + kVPre + k : 0) * kSpan + tid * 8;
          yv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v8h*>(th + e)) : zero;
          rv[k] = in ? __builtin_nontemporal_load(reinterpret_cast<const v8h*>(rh + e)) : zero;
        }
#pragma unroll
        for (int k = 0; k < kVPre; ++k) {
          if (b0 + k >= nfull) break;
#pragma unroll
          for (int q = 0; q < 8; ++q) cell((int)yc[k][q], (int)rc[k][q]);
        }
      }
      cs0 = c0 + nfull * kSpan;
    }
    constexpr int kPre = 4;
    int yb[kPre], rb[kPre];
    const int64_t e0 = cs0 + tid;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      const int64_t e = e0 + (int64_t)k * kHsBlock;
      yb[k] = (e < c1) ? rd(trow, e * by) : 0;
      rb[k] = (e < c1) ? rd(rrow, e * by) : 0;
    }
    for (int64_t e = e0; e < c1; e += (int64_t)kPre * kHsBlock) {
      int yc[kPre], rc[kPre];
#pragma unroll
      for (int k = 0; k < kPre; ++k) { yc[k] = yb[k]; rc[k] = rb[k]; }
#pragma unroll
      for (int k = 0; k < kPre; ++k) {
        const int64_t en = e + (int64_t)(kPre + k) * kHsBlock;
        yb[k] = (en < c1) ? rd(trow, en * by) : 0;
        rb[k] = (en < c1) ? rd(rrow, en * by) : 0;
      }
#pragma unroll
      for (int k = 0; k < kPre; ++k) {
        if (e + (int64_t)k * kHsBlock >= c1) break;
        cell(yc[k], rc[k]);
      }
    }
    if (c1 < E) {   // another chunk follows: the bins that could wrap in it leave the LDS now (a handful per sample at most)
      __syncthreads();
      for (int i = tid; i < kSmBins / 2; i += kHsBlock) {
        uint32_t w = h[i];
        if (w & 0xC000C000u) {
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const uint32_t c = (w >> (16 * hf)) & 0xffffu;
            if (c >= kSmHot) {
              const int k = atomicAdd(&carry_n, 1);
              if (k < kSmCarry) { carry_bin[k] = (uint32_t)(2 * i + hf); carry_cnt[k] = c; }
              w &= ~(0xffffu << (16 * hf));
            }
          }
          h[i] = w;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int v = tid; v < kSmBins; v += kHsBlock) row[v] = (h[v >> 1] >> ((v & 1) * 16)) & 0xffffu;   // the one flush: whole lines
  const int nc = carry_n;
  if (nc > 0) {
    __threadfence();
    __syncthreads();
    for (int k = tid; k < nc && k < kSmCarry; k += kHsBlock) atomicAdd(&row[carry_bin[k]], carry_cnt[k]);
  }
  // (more early movers than the list holds -- millions of cells on a few values: the sample is summed cell by cell, as when a list ran out)
  ovn[s * kHistGroups + tid] = (nc > kSmCarry) ? (int)cap + 1 : nov;
  for (int g = kHsBlock + tid; g < kHistGroups; g += kHsBlock) ovn[s * kHistGroups + g] = 0;
}

// One block of consecutive bins of a count histogram in the Newton sums of k_fit_hnewton.  Consecutive bins are
// consecutive integers, so only the block's first bin is evaluated in full (difference form: psi(x0 + v) - psi(x0) =
// ln((x0 + v)/x0) + (rest - rest0)); from there
//     psi(x + 1) = psi(x) + 1/x,     psi'(x + 1) = psi'(x) - 1/x^2
// carry the two differences along: one reciprocal per bin instead of a digamma, a trigamma and a logarithm.  The psi
// recurrence is summed error-free (TwoSum into a low word), so a bin's value is as accurate as the block's first one;
// for psi' (curvature only) the plain sum's few roundings are immaterial.
// Counts: global histogram halves g0, g1 (one bin every gs words: 4 in the quad layout, 1 in a sample's own row; either may be null) plus packed 16-bit LDS bins
// (l, first bin li; null = none).  x = shape parameter + value of the block's first bin; (ix0, r0, q0) describe the
// reference point x0 as digamma_trigamma_nolog(x0) returns it (1/xs, rest, psi').  Returns (sum c dpsi, sum c dpsi').
__device__ __noinline__ double2 hn_block(double x, int nb, const uint32_t* __restrict__ g0, const uint32_t* __restrict__ g1,
                                         const uint32_t* l, int li, double ix0, double r0, double q0, int gs)
{
  double x1, r1, q1;
  edfit::digamma_trigamma_nolog(x, x1, r1, q1);
  double dh = edfit::flog(x1 * ix0) + (r1 - r0), dl = 0.0;   // psi(x) - psi(x0), high and low word
  double dq = q1 - q0;                                       // psi'(x) - psi'(x0)
  double g = 0.0, h = 0.0;
  constexpr int kChunk = 4;   // counts requested together: bin by bin, every bin waited ~1 us for its own two loads
  // a sample's own row (gs == 1): the block's counts are consecutive words, 16-byte aligned -- all of them requested at once, as
  // 16-byte loads, before the first is used (one round trip to the L2 per block instead of one per four bins)
  typedef unsigned int hn_v4u __attribute__((ext_vector_type(4)));
  constexpr int kMaxQ = 5;    // blocks of up to 20 bins: every block of geometry 8
  hn_v4u pre[kMaxQ];
  const bool rowform = gs == 1 && g1 == nullptr && nb <= 4 * kMaxQ;   // (the deeper geometries' blocks of 32 / 64 bins keep the chunked form)
  if (rowform) {
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q)
      pre[q] = (g0 && 4 * q < nb) ? *reinterpret_cast<const hn_v4u*>(g0 + 4 * q) : hn_v4u{0u, 0u, 0u, 0u};
  }
  for (int k0 = 0; k0 < nb; k0 += kChunk) {   // (nb is a multiple of 4: static_asserts below)
    uint32_t c[kChunk];
    if (rowform) {
      hn_v4u v = pre[0];
#pragma unroll
      for (int q = 1; q < kMaxQ; ++q) if (k0 == 4 * q) v = pre[q];
      c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (l) c[j] += (l[(li + k0 + j) >> 1] >> (((li + k0 + j) & 1) * 16)) & 0xffffu;
    } else
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const int k = k0 + j;
      c[j] = 0;
      if (g0) c[j] += g0[gs * k];
      if (g1) c[j] += g1[gs * k];
      if (l) c[j] += (l[(li + k) >> 1] >> (((li + k) & 1) * 16)) & 0xffffu;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const double cd = (double)c[j];
      g = __builtin_fma(cd, dh + dl, g);
      h = __builtin_fma(cd, dq, h);
      const double r = edfit::frcp(x + (double)(k0 + j));
      const double t = dh + r;                                 // TwoSum(dh, r)
      const double bb = t - dh;
      dl += (dh - (t - bb)) + (r - bb);
      dh = t;
      dq = __builtin_fma(-r, r, dq);
    }
  }
  return make_double2(g, h);
}



// ---- fit mode 1 ("aod-nm"): the reference's own procedure on the same histograms ---------------------------------
// aod::betabin (R/class_definition.R:118; aod 1.3, a CRAN package outside the reference tree -- restated from its documented
// algorithm, parity unpinned) minimises
//     -sum_e [ lchoose(n_e, y_e) + lbeta(a + y_e, b + n_e - y_e) - lbeta(a, b) ],   a = p (1 - phi)/phi, b = (1 - p)(1 - phi)/phi,
//     p = plogis(beta),  value 1e20 where the sum is not finite (phi outside (0, 1))
// over (beta, phi) with optim()'s default method from (glm-binomial intercept, 0.1): R's nmmin (src/appl/optim.c; Nelder-Mead as in
// Nash, Compact Numerical Methods, algorithm 19) with alpha = 1, beta = 0.5, gamma = 2, abstol = -Inf, reltol = sqrt(eps) and
// maxit = 2000 function evaluations.  Every term is a function of ONE count, lbeta(a + y, b + r) - lbeta(a, b) =
// D(a, y) + D(b, r) - D(a + b, y + r) with D(x, v) = lgamma(x + v) - lgamma(x), so the objective is a sum over the bins of the
// three count histograms; consecutive bins are consecutive integers and D(x, v + 1) = D(x, v) + ln(x + v): one logarithm per bin.
// The binomial coefficients are a constant of the data (they only scale optim's relative tolerance): the same sum at a = b = 1.

// lgamma(x) for x > 0: recurrence up to x >= 12, then Stirling's series (|error| < 1e-15 relative)
__device__ __forceinline__ double nm_lgamma(double x)
{
  double shift = 0.0;
  while (x < 12.0) { shift += edfit::flog(x); x += 1.0; }
  const double r = edfit::frcp(x), w = r * r;
  double s = -691.0 / 360360.0;
  s = ed_pm_fma_k(s, w, 1.0 / 1188.0);
  s = ed_pm_fma_k(s, w, -1.0 / 1680.0);
  s = ed_pm_fma_k(s, w, 1.0 / 1260.0);
  s = ed_pm_fma_k(s, w, -1.0 / 360.0);
  s = ed_pm_fma_k(s, w, 1.0 / 12.0);
  return ((x - 0.5) * edfit::flog(x) - x + 0.91893853320467274178) + s * r - shift;
}
// D(x, v) = lgamma(x + v) - lgamma(x), v >= 0 an integer
__device__ __forceinline__ double nm_D(double x, int v)
{
  if (v <= 0) return 0.0;
  if (v <= 8) { double d = 0.0; for (int k = 0; k < v; ++k) d += edfit::flog(x + (double)k); return d; }
  return nm_lgamma(x + (double)v) - nm_lgamma(x);
}
// sum over one block of consecutive bins of count * D(x0, v); counts as in hn_block
__device__ __noinline__ double nm_block(double x0, int v0, int nb, const uint32_t* __restrict__ g0, const uint32_t* __restrict__ g1,
                                        const uint32_t* l, int li, int gs)
{
  double D = nm_D(x0, v0), acc = 0.0;
  constexpr int kChunk = 4;
  for (int k0 = 0; k0 < nb; k0 += kChunk) {
    uint32_t c[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const int k = k0 + j;
      c[j] = 0;
      if (g0) c[j] += g0[gs * k];
      if (g1) c[j] += g1[gs * k];
      if (l) c[j] += (l[(li + k) >> 1] >> (((li + k) & 1) * 16)) & 0xffffu;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      acc = __builtin_fma((double)c[j], D, acc);
      D += edfit::flog(x0 + (double)(v0 + k0 + j));
    }
  }
  return acc;
}

// nmmin's state for one sample (kept by strand 0)
struct NmState {
  double P[2][4];      // P[i][j]: coordinate i of vertex j = 0..2, column 3 = centroid / work point
  double F[4];         // function values of the columns
  double B[2];         // the point being evaluated (Bvec)
  double convtol, oldsize, VL, VH, VR, lc;
  int L, H, funcount, phase, j, fail;   // phase: what the pending evaluation is for
};
enum { NM_LC = 0, NM_START, NM_VERT, NM_REFLECT, NM_EXTEND, NM_CONTRACT, NM_DONE };

__device__ __forceinline__ void nm_point(const NmState& st, double& a, double& b, double& th, bool& valid)
{
  if (st.phase == NM_LC) { a = b = 1.0; th = 1.0; valid = true; return; }
  const double beta = st.B[0], phi = st.B[1];
  valid = (phi > 0.0 && phi < 1.0) && (beta == beta) && fabs(beta) < 700.0;
  const double p = 1.0 / (1.0 + ed_pexp(-beta));
  const double k = (1.0 - phi) / phi;
  a = p * k; b = (1.0 - p) * k; th = a + b;
  valid = valid && a > 0.0 && b > 0.0 && th < 1e300;
  if (!valid) { a = b = 1.0; th = 2.0; }
}

// next vertex the calcvert loop has to evaluate (j != L - 1), or -1
__device__ __forceinline__ int nm_next_vertex(const NmState& st, int from)
{
  for (int j = from; j < 3; ++j) if (j + 1 != st.L) return j;
  return -1;
}

// after the vertices are known: order, test for convergence, reflect.  Returns with st.phase = NM_REFLECT and st.B set, or NM_DONE.
__device__ __forceinline__ void nm_iterate(NmState& st, int maxit)
{
  if (st.funcount > maxit) { st.fail = 1; st.phase = NM_DONE; return; }
  st.VL = st.F[st.L - 1]; st.VH = st.VL; st.H = st.L;
  for (int j = 1; j <= 3; ++j) {
    if (j != st.L) {
      const double f = st.F[j - 1];
      if (f < st.VL) { st.L = j; st.VL = f; }
      if (f > st.VH) { st.H = j; st.VH = f; }
    }
  }
  if (st.VH <= st.VL + st.convtol) { st.phase = NM_DONE; return; }
  for (int i = 0; i < 2; ++i) {
    double temp = -st.P[i][st.H - 1];
    for (int j = 0; j < 3; ++j) temp += st.P[i][j];
    st.P[i][3] = temp / 2.0;
  }
  for (int i = 0; i < 2; ++i) st.B[i] = (1.0 + 1.0) * st.P[i][3] - 1.0 * st.P[i][st.H - 1];
  st.phase = NM_REFLECT;
}

// consume the value f of the pending evaluation; leaves the next evaluation in (st.phase, st.B) or NM_DONE
__device__ __noinline__ void nm_advance(NmState& st, double f, double b0, int maxit)
{
  const double big = 1.0e+35, bet = 0.5, gamm = 2.0, intol = 1.490116119384765625e-08;
  switch (st.phase) {
    case NM_LC:
      st.lc = -f;                       // sum of lchoose(n, y)
      st.B[0] = b0; st.B[1] = 0.1;      // aod's start: glm-binomial intercept, phi = 0.1
      st.phase = NM_START;
      return;
    case NM_START: {
      if (!(fabs(f) <= 1.7976931348623157e308)) { st.fail = 2; st.phase = NM_DONE; st.P[0][0] = b0; st.P[1][0] = 0.1; st.L = 1; return; }
      st.funcount = 1;
      st.convtol = intol * (fabs(f) + intol);
      st.F[0] = f;
      st.P[0][0] = st.B[0]; st.P[1][0] = st.B[1];
      st.L = 1;
      double size = 0.0, step = 0.0;
      for (int i = 0; i < 2; ++i) if (0.1 * fabs(st.B[i]) > step) step = 0.1 * fabs(st.B[i]);
      if (step == 0.0) step = 0.1;
      for (int j = 2; j <= 3; ++j) {
        for (int i = 0; i < 2; ++i) st.P[i][j - 1] = st.B[i];
        double trystep = step;
        while (st.P[j - 2][j - 1] == st.B[j - 2]) { st.P[j - 2][j - 1] = st.B[j - 2] + trystep; trystep *= 10; }
        size += trystep;
      }
      st.oldsize = size;
      st.j = nm_next_vertex(st, 0);
      st.B[0] = st.P[0][st.j]; st.B[1] = st.P[1][st.j];
      st.phase = NM_VERT;
      return;
    }
    case NM_VERT: {
      st.F[st.j] = (fabs(f) <= 1.7976931348623157e308) ? f : big;
      ++st.funcount;
      const int nx = nm_next_vertex(st, st.j + 1);
      if (nx >= 0) { st.j = nx; st.B[0] = st.P[0][nx]; st.B[1] = st.P[1][nx]; return; }
      nm_iterate(st, maxit);
      return;
    }
    case NM_REFLECT: {
      if (!(fabs(f) <= 1.7976931348623157e308)) f = big;
      ++st.funcount;
      st.VR = f;
      if (st.VR < st.VL) {
        st.F[3] = f;
        for (int i = 0; i < 2; ++i) {
          const double t = gamm * st.B[i] + (1 - gamm) * st.P[i][3];
          st.P[i][3] = st.B[i];
          st.B[i] = t;
        }
        st.phase = NM_EXTEND;
        return;
      }
      if (st.VR < st.VH) {
        for (int i = 0; i < 2; ++i) st.P[i][st.H - 1] = st.B[i];
        st.F[st.H - 1] = st.VR;
      }
      for (int i = 0; i < 2; ++i) st.B[i] = (1 - bet) * st.P[i][st.H - 1] + bet * st.P[i][3];
      st.phase = NM_CONTRACT;
      return;
    }
    case NM_EXTEND: {
      if (!(fabs(f) <= 1.7976931348623157e308)) f = big;
      ++st.funcount;
      if (f < st.VR) {
        for (int i = 0; i < 2; ++i) st.P[i][st.H - 1] = st.B[i];
        st.F[st.H - 1] = f;
      } else {
        for (int i = 0; i < 2; ++i) st.P[i][st.H - 1] = st.P[i][3];
        st.F[st.H - 1] = st.VR;
      }
      nm_iterate(st, maxit);
      return;
    }
    case NM_CONTRACT: {
      if (!(fabs(f) <= 1.7976931348623157e308)) f = big;
      ++st.funcount;
      if (f < st.F[st.H - 1]) {
        for (int i = 0; i < 2; ++i) st.P[i][st.H - 1] = st.B[i];
        st.F[st.H - 1] = f;
      } else if (st.VR >= st.VH) {
        double size = 0.0;
        for (int j = 0; j < 3; ++j) {
          if (j + 1 != st.L) {
            for (int i = 0; i < 2; ++i) {
              st.P[i][j] = bet * (st.P[i][j] - st.P[i][st.L - 1]) + st.P[i][st.L - 1];
              size += fabs(st.P[i][j] - st.P[i][st.L - 1]);
            }
          }
        }
        if (size < st.oldsize) {
          st.oldsize = size;
          if (st.funcount > maxit) { st.fail = 1; st.phase = NM_DONE; return; }
          st.j = nm_next_vertex(st, 0);
          st.B[0] = st.P[0][st.j]; st.B[1] = st.P[1][st.j];
          st.phase = NM_VERT;
          return;
        }
        st.fail = 10; st.phase = NM_DONE;
        return;
      }
      nm_iterate(st, maxit);
      return;
    }
    default: return;
  }
}

// All Newton iterations of 4 samples in one launch: 256 strands per sample share the bins and the overflow
// regions (strand y: bins y, y + 256, ...; row group y), a fixed-order LDS tree adds them up,
// strand 0 takes the step.
constexpr int kHnS = 4;    // samples per workgroup
constexpr int kHnY = 256;  // strands per sample
static_assert(kHistGroups % kHnY == 0, "every strand owns whole overflow regions");
static_assert(kHnS == 4 && kHistHalves == 2, "hist_at's quads");
static_assert(kHistKy % (4 * kHnY) == 0 && kHistKr % (4 * kHnY) == 0 && kHistKn % (4 * kHnY) == 0 && kOv2 % (4 * kHnY) == 0, "whole blocks of whole chunks per strand");

__global__ void __launch_bounds__(kHnS * kHnY)
k_fit_hnewton(const uint32_t* __restrict__ hist, int32_t* __restrict__ ov_y, int32_t* __restrict__ ov_r,
              const int32_t* __restrict__ ovn, int64_t cap, int64_t S, double* __restrict__ eta, double* __restrict__ lam,
              int* __restrict__ done, int max_iter, double tol, const int32_t* __restrict__ test,
              const int32_t* __restrict__ ref, int64_t rs, int64_t E, const int* __restrict__ depth_max, int launched, int64_t cs,
              double* __restrict__ phi_out, double* __restrict__ exp_out,   // (non-null: k_fit_finish's two lines, saving its launch)
              int lay,   // 0: k_fit_hist's quads and halves, lists [slot][S]; 1: k_fit_hist_sm's rows, lists [S][slot]
              int cb)    // bytes per count of test / ref (read only by a sample whose lists ran out)
{
  if (!fit_hist_runs(*depth_max, launched, kHistId)) return;
  __shared__ double lds[kFitQ][kHnY][kHnS];
  __shared__ double sh_eta[kHnS], sh_lam[kHnS];
  __shared__ int sh_done[kHnS], sh_over[kHnS];
  __shared__ uint32_t ov2[kHnS][kOv2Words];
  __shared__ int res_pre[kHnS][kHistGroups + 1];   // exclusive prefix over the lists of the cells still evaluated one by one
  const int lane = threadIdx.x, y = threadIdx.y;
  for (int i = y * kHnS + lane; i < kHnS * kOv2Words; i += kHnS * kHnY) (&ov2[0][0])[i] = 0u;
  const int64_t s = (int64_t)blockIdx.x * kHnS + lane;
  const bool live = s < S;
  const int64_t sc = live ? s : S - 1;
  const int64_t Sp = hist_padded(S);
  const int gs = lay ? 1 : 4;
  const uint32_t* __restrict__ rowp = hist + sc * kSmBins;
  auto G0 = [&](int v) -> const uint32_t* { return lay ? rowp + v : hist + hist_at(0, v, sc, Sp); };
  auto G1 = [&](int v) -> const uint32_t* { return lay ? (const uint32_t*)nullptr : hist + hist_at(1, v, sc, Sp); };
  auto G2 = [&](int off) -> const uint32_t* { return (lay && kSm2) ? rowp + kHistK + off : (const uint32_t*)nullptr; };   // the second level k_fit_hist_sm filled
  auto OV = [&](int64_t slot) -> int64_t { return lay ? sc * ((int64_t)kHistGroups * cap) + slot : slot * S + sc; };
  if (y == 0) sh_over[lane] = 0;
  __syncthreads();
  int cnt[kHistGroups / kHnY];
  bool over = false;
#pragma unroll
  for (int k = 0; k < kHistGroups / kHnY; ++k) {
    cnt[k] = lay ? ovn[sc * kHistGroups + (y + k * kHnY)] : ovn[(int64_t)(y + k * kHnY) * S + sc];
    over |= cnt[k] > cap;
  }
  if (over) atomicOr(&sh_over[lane], 1);
  __syncthreads();
  const bool fits = !sh_over[lane];            // otherwise (an overflow region ran out) the sample is summed cell by cell
  if (y == 0) {
    sh_eta[lane] = eta[sc];
    sh_lam[lane] = lam[sc];
    sh_done[lane] = live ? done[sc] : 1;
  }
  __syncthreads();
  // second-level bins from the overflow lists (16-bit: kHistGroups lists of at most cap cells, kHistGroups x cap < 65536)
  if (fits && !sh_done[lane]) {
#pragma unroll
    for (int k = 0; k < kHistGroups / kHnY; ++k) {
      const int64_t base = (int64_t)(y + k * kHnY) * cap;
      int nres = 0;
      for (int i = 0; i < cnt[k]; ++i) {
        const int yy = ov_y[OV(base + i)], rr = ov_r[OV(base + i)];
        const unsigned ri = (unsigned)(rr - kOv2R0), ni = (unsigned)(yy + rr - kHistKn);
        if ((unsigned)yy < (unsigned)kHistKy && ri < (unsigned)kOv2 && ni < (unsigned)kOv2) {
          const int by = yy, br = kHistKy + (int)ri, bn = kHistKy + kOv2 + (int)ni;
          atomicAdd(&ov2[lane][by >> 1], 1u << ((by & 1) * 16));
          atomicAdd(&ov2[lane][br >> 1], 1u << ((br & 1) * 16));
          atomicAdd(&ov2[lane][bn >> 1], 1u << ((bn & 1) * 16));
        } else {
          if (nres != i) { ov_y[OV(base + nres)] = yy; ov_r[OV(base + nres)] = rr; }   // this strand's list only
          ++nres;
        }
      }
      cnt[k] = nres;
    }
  }
#pragma unroll
  for (int k = 0; k < kHistGroups / kHnY; ++k) res_pre[lane][y + k * kHnY + 1] = (fits && !sh_done[lane]) ? cnt[k] : 0;
  __syncthreads();
  if (y == 0) {
    int run = 0;
    res_pre[lane][0] = 0;
    for (int g = 1; g <= kHistGroups; ++g) { run += res_pre[lane][g]; res_pre[lane][g] = run; }
  }
  __syncthreads();
  for (int it = 0; it < max_iter; ++it) {
    const int dn = sh_done[lane];
    if (__syncthreads_and(dn)) break;
    double acc[kFitQ];
#pragma unroll
    for (int q = 0; q < kFitQ; ++q) acc[q] = 0.0;
    if (!dn && !fits) {
      // rare: the plain per-cell sums (raw psi values, the cell count in acc[5] lets fit_newton_step subtract the
      // constant terms), the strands sharing the rows
      const double th = ed_pexp(sh_lam[lane]);
      const double p = 1.0 / (1.0 + ed_pexp(-sh_eta[lane]));
      const double a = th * p, b = th * (1.0 - p);
      // (deep data -- counts beyond every geometry's bins, round 6's regime map at 1 600 reads per exon -- take this path for every cell and iteration:
      //  one logarithm per run of eight cells, as k_fit_accum (ed_fit_dev.hpp).  The short digamma / trigamma series of that kernel is NOT used here: with it
      //  -- per lane or per wave, the values bit for bit the long series' (ed_eval_sf 15 - 18) -- this kernel's fits came out wrong now and then, run to
      //  run, in tests/test_gpu_fit.py (5 runs: 3 with failures; without: 10 of 10 clean).  The kernel sits at its 128-register cap with 256-288 bytes of
      //  scratch per lane; the cause was not found in the time there was, so the path that was stable stays.)
      edfit::Acc c = {0, 0, 0, 0, 0};
      double n_cells = 0.0, pa = 1.0, pb = 1.0;
      int in_run = 0;
      for (int64_t e = y; e < E; e += kHnY) {
        const int yy = ed_ldc(test, e * rs + sc * cs, cb), rr = ed_ldc(ref, e * rs + sc * cs, cb);     // (rs, cs) = (row pitch, 1): [E][S]; (1, row pitch): [S][E]
        if (yy + rr > 0) {
#ifdef ED_HN_SHORT_SERIES   // (diagnostic build `hnshort`: the variant whose fits were not reproducible from run to run -- see the comment above)
          edfit::accumulate_cell_run(c, pa, pb, a, b, th, yy, yy + rr, a + (double)yy >= 32.0 && b + (double)rr >= 32.0);
#else
          edfit::accumulate_cell_run(c, pa, pb, a, b, th, yy, yy + rr, false);
#endif
          n_cells += 1.0;
          if (++in_run == 8) { c.ga += edfit::flog(pa); c.gb += edfit::flog(pb); pa = pb = 1.0; in_run = 0; }
        }
      }
      c.ga += edfit::flog(pa); c.gb += edfit::flog(pb);
      acc[0] = c.ga; acc[1] = c.gb; acc[2] = c.haa; acc[3] = c.hab; acc[4] = c.hbb; acc[5] = n_cells;
    } else if (!dn) {
      const double th = ed_pexp(sh_lam[lane]);
      const double p = 1.0 / (1.0 + ed_pexp(-sh_eta[lane]));
      const double a = th * p, b = th * (1.0 - p);
      // The sums are formed from DIFFERENCES psi(a + v) - psi(a) = ln((a + v)/a) + (rest(a + v) - rest(a)) (and the
      // same for b, a + b and for psi'): the constant terms of the gradient are folded in bin by bin instead of being
      // subtracted from a sum ~1/phi times larger at the end, which cost 1/phi in relative accuracy (seen as 1e-5
      // on phi at phi = 5e-5 with the plain sums).
      double xa, ra, qa, xb, rb, qb, xt, rt, qt;
      edfit::digamma_trigamma_nolog(a, xa, ra, qa);
      edfit::digamma_trigamma_nolog(b, xb, rb, qb);
      edfit::digamma_trigamma_nolog(th, xt, rt, qt);
      const double ixa = edfit::frcp(xa), ixb = edfit::frcp(xb), ixt = edfit::frcp(xt);
      // a strand owns a block of consecutive bins of each histogram (first level 4 / 16 / 16, second level 20 / 20)
      {
        constexpr int nb = kHistKy / kHnY;
        const double2 t = hn_block(a + (double)(y * nb), nb, G0(y * nb), G1(y * nb), ov2[lane], y * nb, ixa, ra, qa, gs);
        acc[0] += t.x; acc[2] += t.y;
      }
      {
        constexpr int nb = kHistKr / kHnY;
        const double2 t = hn_block(b + (double)(y * nb), nb, G0(kHistKy + y * nb), G1(kHistKy + y * nb), nullptr, 0, ixb, rb, qb, gs);
        acc[1] += t.x; acc[4] += t.y;
      }
      {
        constexpr int nb = kHistKn / kHnY;
        const double2 t = hn_block(th + (double)(y * nb), nb, G0(kHistKy + kHistKr + y * nb), G1(kHistKy + kHistKr + y * nb), nullptr, 0, ixt, rt, qt, gs);
        acc[0] -= t.x; acc[1] -= t.x;
        acc[2] -= t.y; acc[3] -= t.y; acc[4] -= t.y;
      }
      {
        constexpr int nb = kOv2 / kHnY;
        const double2 tr = hn_block(b + (double)(kOv2R0 + y * nb), nb, G2(y * nb), nullptr, ov2[lane], kHistKy + y * nb, ixb, rb, qb, 1);
        acc[1] += tr.x; acc[4] += tr.y;
        const double2 t = hn_block(th + (double)(kHistKn + y * nb), nb, G2(kOv2 + y * nb), nullptr, ov2[lane], kHistKy + kOv2 + y * nb, ixt, rt, qt, 1);
        acc[0] -= t.x; acc[1] -= t.x;
        acc[2] -= t.y; acc[3] -= t.y; acc[4] -= t.y;
      }
      // cells beyond the bins: evaluated whole, minus the same constant terms
      const double ca = edfit::flog(xa * ixt) + (ra - rt), cb = edfit::flog(xb * ixt) + (rb - rt);
      // the lists differ in length (a few cells each, Poisson): walked list by list, a wave would take as long as its
      // longest list; instead the strands share the concatenation of the sample's lists round-robin
      const int n_res = res_pre[lane][kHistGroups];
      for (int q = y; q < n_res; q += kHnY) {
        int lo_g = 0, hi_g = kHistGroups;   // which list holds cell q of the concatenation?
        while (hi_g - lo_g > 1) {
          const int mid = (lo_g + hi_g) >> 1;
          if (res_pre[lane][mid] <= q) lo_g = mid; else hi_g = mid;
        }
        const int64_t slot = (int64_t)lo_g * cap + (q - res_pre[lane][lo_g]);
        const int yy = ov_y[OV(slot)], rr = ov_r[OV(slot)];
        edfit::Acc c = {0, 0, 0, 0, 0};
        double pa = 1.0, pb = 1.0;
        edfit::accumulate_cell_run(c, pa, pb, a, b, th, yy, yy + rr, false);
        c.ga += edfit::flog(pa); c.gb += edfit::flog(pb);
        acc[0] += c.ga - ca; acc[1] += c.gb - cb; acc[2] += c.haa - (qa - qt); acc[3] += c.hab + qt; acc[4] += c.hbb - (qb - qt);
      }
    }
    // acc[5] (the cell count that scales the constant terms in fit_newton_step) stays 0: they are already in
#pragma unroll
    for (int q = 0; q < kFitQ; ++q) lds[q][y][lane] = acc[q];
    __syncthreads();
    for (int hh = kHnY / 2; hh >= 1; hh >>= 1) {
      if (y < hh) {
#pragma unroll
        for (int q = 0; q < kFitQ; ++q) lds[q][y][lane] += lds[q][y + hh][lane];
      }
      __syncthreads();
    }
    if (y == 0 && !dn) {
      double tot[kFitQ];
#pragma unroll
      for (int q = 0; q < kFitQ; ++q) tot[q] = lds[q][0][lane];
      double e = sh_eta[lane], l = sh_lam[lane];
      int d = 0;
      fit_newton_step(tot, e, l, d, tol, 1);
      sh_eta[lane] = e; sh_lam[lane] = l; sh_done[lane] = d;
    }
    __syncthreads();
  }
  if (y == 0 && live) {
    eta[s] = sh_eta[lane];
    lam[s] = sh_lam[lane];
    done[s] = sh_done[lane];
    if (phi_out) {
      phi_out[s] = 1.0 / (ed_pexp(sh_lam[lane]) + 1.0);
      exp_out[s] = 1.0 / (1.0 + ed_pexp(-sh_eta[lane]));
    }
  }
}


// Fit mode 1: the whole Nelder-Mead search of 4 samples in one launch -- same geometry as k_fit_hnewton (256 strands per
// sample share the bins; a fixed-order LDS tree adds them up); strand 0 of a sample runs nmmin's state machine and publishes
// the next point to evaluate.  On entry eta[] holds logit(sum y / sum n) (k_fit_start): aod's glm-binomial start.
__global__ void __launch_bounds__(kHnS * kHnY)
k_fit_hnm(const uint32_t* __restrict__ hist, int32_t* __restrict__ ov_y, int32_t* __restrict__ ov_r,
          const int32_t* __restrict__ ovn, int64_t cap, int64_t S, double* __restrict__ eta, double* __restrict__ lam,
          int* __restrict__ done, int maxit, const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t rs, int64_t E,
          const int* __restrict__ depth_max, int launched, int* __restrict__ fevals, int64_t cs, double* __restrict__ phi_out,
          double* __restrict__ exp_out, int lay, int cb)
{
  if (!fit_hist_runs(*depth_max, launched, kHistId)) return;
  __shared__ double lds[kHnY][kHnS];
  __shared__ double sh_q[kHnS][3];
  __shared__ int sh_flag[kHnS];                 // bit 0: an evaluation is pending, bit 1: the point is inside the domain
  __shared__ int sh_over[kHnS];
  __shared__ uint32_t ov2[kHnS][kOv2Words];
  __shared__ int res_pre[kHnS][kHistGroups + 1];
  const int lane = threadIdx.x, y = threadIdx.y;
  for (int i = y * kHnS + lane; i < kHnS * kOv2Words; i += kHnS * kHnY) (&ov2[0][0])[i] = 0u;
  const int64_t s = (int64_t)blockIdx.x * kHnS + lane;
  const bool live = s < S;
  const int64_t sc = live ? s : S - 1;
  const int64_t Sp = hist_padded(S);
  const int gs = lay ? 1 : 4;
  const uint32_t* __restrict__ rowp = hist + sc * kSmBins;
  auto G0 = [&](int v) -> const uint32_t* { return lay ? rowp + v : hist + hist_at(0, v, sc, Sp); };
  auto G1 = [&](int v) -> const uint32_t* { return lay ? (const uint32_t*)nullptr : hist + hist_at(1, v, sc, Sp); };
  auto G2 = [&](int off) -> const uint32_t* { return (lay && kSm2) ? rowp + kHistK + off : (const uint32_t*)nullptr; };   // the second level k_fit_hist_sm filled
  auto OV = [&](int64_t slot) -> int64_t { return lay ? sc * ((int64_t)kHistGroups * cap) + slot : slot * S + sc; };
  if (y == 0) sh_over[lane] = 0;
  __syncthreads();
  int cnt[kHistGroups / kHnY];
  bool over = false;
#pragma unroll
  for (int k = 0; k < kHistGroups / kHnY; ++k) {
    cnt[k] = lay ? ovn[sc * kHistGroups + (y + k * kHnY)] : ovn[(int64_t)(y + k * kHnY) * S + sc];
    over |= cnt[k] > cap;
  }
  if (over) atomicOr(&sh_over[lane], 1);
  __syncthreads();
  const bool fits = !sh_over[lane];
  const bool skip = !live || done[sc];          // done = 1 on entry: nothing to fit (k_fit_start)
  // second-level bins from the overflow lists, as k_fit_hnewton builds them
  if (fits && !skip) {
#pragma unroll
    for (int k = 0; k < kHistGroups / kHnY; ++k) {
      const int64_t base = (int64_t)(y + k * kHnY) * cap;
      int nres = 0;
      for (int i = 0; i < cnt[k]; ++i) {
        const int yy = ov_y[OV(base + i)], rr = ov_r[OV(base + i)];
        const unsigned ri = (unsigned)(rr - kOv2R0), ni = (unsigned)(yy + rr - kHistKn);
        if ((unsigned)yy < (unsigned)kHistKy && ri < (unsigned)kOv2 && ni < (unsigned)kOv2) {
          const int by = yy, br = kHistKy + (int)ri, bn = kHistKy + kOv2 + (int)ni;
          atomicAdd(&ov2[lane][by >> 1], 1u << ((by & 1) * 16));
          atomicAdd(&ov2[lane][br >> 1], 1u << ((br & 1) * 16));
          atomicAdd(&ov2[lane][bn >> 1], 1u << ((bn & 1) * 16));
        } else {
          if (nres != i) { ov_y[OV(base + nres)] = yy; ov_r[OV(base + nres)] = rr; }
          ++nres;
        }
      }
      cnt[k] = nres;
    }
  }
#pragma unroll
  for (int k = 0; k < kHistGroups / kHnY; ++k) res_pre[lane][y + k * kHnY + 1] = (fits && !skip) ? cnt[k] : 0;
  __syncthreads();
  if (y == 0) {
    int run = 0;
    res_pre[lane][0] = 0;
    for (int g = 1; g <= kHistGroups; ++g) { run += res_pre[lane][g]; res_pre[lane][g] = run; }
  }
  NmState st;
  st.phase = skip ? NM_DONE : NM_LC;
  st.fail = 0; st.funcount = 0; st.L = 1; st.lc = 0.0;
  st.P[0][0] = eta[sc]; st.P[1][0] = 0.1; st.B[0] = st.P[0][0]; st.B[1] = 0.1;
  const double b0 = eta[sc];
  __syncthreads();
  for (int it = 0; it < maxit + 64; ++it) {
    if (y == 0) {
      double a, b, th;
      bool valid = false;
      const bool pending = st.phase != NM_DONE;
      if (pending) nm_point(st, a, b, th, valid); else { a = b = 1.0; th = 2.0; }
      sh_q[lane][0] = a; sh_q[lane][1] = b; sh_q[lane][2] = th;
      sh_flag[lane] = (pending ? 1 : 0) | (valid ? 2 : 0);
    }
    __syncthreads();
    const int flag = sh_flag[lane];
    if (__syncthreads_and(!(flag & 1))) break;
    double part = 0.0;
    if ((flag & 3) == 3) {
      const double a = sh_q[lane][0], b = sh_q[lane][1], th = sh_q[lane][2];
      if (!fits) {
        for (int64_t e = y; e < E; e += kHnY) {
          const int yy = ed_ldc(test, e * rs + sc * cs, cb), rr = ed_ldc(ref, e * rs + sc * cs, cb);
          if (yy + rr > 0) part += (nm_D(a, yy) + nm_D(b, rr)) - nm_D(th, yy + rr);
        }
      } else {
        {
          constexpr int nb = kHistKy / kHnY;
          part += nm_block(a, y * nb, nb, G0(y * nb), G1(y * nb), ov2[lane], y * nb, gs);
        }
        {
          constexpr int nb = kHistKr / kHnY;
          part += nm_block(b, y * nb, nb, G0(kHistKy + y * nb), G1(kHistKy + y * nb), nullptr, 0, gs);
        }
        {
          constexpr int nb = kHistKn / kHnY;
          part -= nm_block(th, y * nb, nb, G0(kHistKy + kHistKr + y * nb), G1(kHistKy + kHistKr + y * nb), nullptr, 0, gs);
        }
        {
          constexpr int nb = kOv2 / kHnY;
          part += nm_block(b, kOv2R0 + y * nb, nb, G2(y * nb), nullptr, ov2[lane], kHistKy + y * nb, 1);
          part -= nm_block(th, kHistKn + y * nb, nb, G2(kOv2 + y * nb), nullptr, ov2[lane], kHistKy + kOv2 + y * nb, 1);
        }
        const int n_res = res_pre[lane][kHistGroups];
        for (int q = y; q < n_res; q += kHnY) {
          int lo_g = 0, hi_g = kHistGroups;
          while (hi_g - lo_g > 1) {
            const int mid = (lo_g + hi_g) >> 1;
            if (res_pre[lane][mid] <= q) lo_g = mid; else hi_g = mid;
          }
          const int64_t slot = (int64_t)lo_g * cap + (q - res_pre[lane][lo_g]);
          const int yy = ov_y[OV(slot)], rr = ov_r[OV(slot)];
          part += (nm_D(a, yy) + nm_D(b, rr)) - nm_D(th, yy + rr);
        }
      }
    }
    lds[y][lane] = part;
    __syncthreads();
    for (int hh = kHnY / 2; hh >= 1; hh >>= 1) {
      if (y < hh) lds[y][lane] += lds[y + hh][lane];
      __syncthreads();
    }
    if (y == 0 && (flag & 1)) {
      const double tot = lds[0][lane];
      double f;
      if (st.phase == NM_LC) f = tot;
      else {
        f = (flag & 2) ? -(st.lc + tot) : 1e20;                  // aod: a sum that is not finite counts as -1e20
        if (!(fabs(f) <= 1.7976931348623157e308)) f = 1e20;
      }
      nm_advance(st, f, b0, maxit);
    }
    __syncthreads();
  }
  if (y == 0 && live && !skip) {
    const double beta = st.P[0][st.L - 1], phi = st.P[1][st.L - 1];
    eta[s] = beta;
    lam[s] = edfit::flog((1.0 - phi) / phi);                     // k_fit_finish: phi = 1 / (exp(lam) + 1)
    done[s] = (st.fail == 0 && st.phase == NM_DONE) ? 1 : 0;
    if (fevals) fevals[s] = st.funcount;
  }
  if (y == 0 && live && phi_out) {     // k_fit_finish's two lines (the samples that were skipped keep k_fit_start's values)
    phi_out[s] = 1.0 / (ed_pexp(lam[s]) + 1.0);
    exp_out[s] = 1.0 / (1.0 + ed_pexp(-eta[s]));
  }
}

// ---- host side: this geometry's launches (fit_columns calls them for hg8, hg4, hg2 in turn) ----
struct Launch {
  static constexpr int kIndex = kHistId == 8 ? 0 : (kHistId == 4 ? 1 : 2);   // this geometry's place in the workspace's caps
  // cells per (row group, sample) list for fits of up to E rows: ~1/3 of the group's rows, and lists x cap < 65536 (the 16-bit second-level bins
  // of k_fit_hnewton count the cells of all lists of a sample)
  static int64_t cap_of(int64_t E) { return std::min<int64_t>(65535 / kHistGroups, std::max<int64_t>(8, (E / kHistGroups) / 3 + 1)); }
  static bool on(const FitHistArgs& a) { return (a.launched & fit_hist_bit(kHistId)) != 0; }
  static void hist(const FitHistArgs& a)
  {
    const FitJob& j = a.j;
    if (j.sample_major())
      hipLaunchKernelGGL(k_fit_hist_sm, dim3((unsigned)j.S), dim3(kHsBlock), 0, a.st, j.test, j.ref, j.sm_pitch, j.trs, j.E, j.S, a.hist, a.ov_y, a.ov_r,
                         a.ovn, a.cap[kIndex], a.depth, a.launched, j.cb);
    else
      hipLaunchKernelGGL(k_fit_hist, dim3((unsigned)((((j.S + kHistSamples - 1) / kHistSamples * kHistHalves + 7) / 8) * 8)), dim3(kHistBlock), 0, a.st,
                         j.test, j.ref, j.rrs, j.E, j.S, a.hist, a.ov_y, a.ov_r, a.ovn, a.cap[kIndex], a.depth, a.launched);
  }
  static void nm(const FitHistArgs& a)
  {
    const FitJob& j = a.j;
    hipLaunchKernelGGL(k_fit_hnm, dim3((unsigned)((j.S + kHnS - 1) / kHnS)), dim3(kHnS, kHnY), 0, a.st, a.hist, a.ov_y, a.ov_r, a.ovn, a.cap[kIndex], j.S,
                       a.eta, a.lam, a.done, 2000 /* optim(control = list(maxit = 2000)) */, j.test, j.ref, a.cell_rs(), j.E, a.depth, a.launched,
                       a.fevals, a.cell_cs(), j.phi, j.expected, j.sample_major() ? 1 : 0, j.cb);
  }
  static void newton(const FitHistArgs& a)
  {
    const FitJob& j = a.j;
    hipLaunchKernelGGL(k_fit_hnewton, dim3((unsigned)((j.S + kHnS - 1) / kHnS)), dim3(kHnS, kHnY), 0, a.st, a.hist, a.ov_y, a.ov_r, a.ovn, a.cap[kIndex], j.S,
                       a.eta, a.lam, a.done, 100, 1e-9 /* iterations are cheap here: converge tightly */, j.test, j.ref, a.cell_rs(), j.E, a.depth,
                       a.launched, a.cell_cs(), j.phi, j.expected, j.sample_major() ? 1 : 0, j.cb);
  }
};
