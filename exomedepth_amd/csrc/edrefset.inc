// edrefset.inc -- select.reference.set on the GPU (included at the end of edcore.hip).
//
// Reference: R/optimize_reference_set.R:53-148 (+ get.power.betabinom, R/tools.R:128-166).  What the R code
// does, and how it is laid out here (R refs, E bins; all matrices [bin][ref], ref-minor):
//   :79-88   total = rowSums(refs) + test; keep bins with total > 30, total < q90(total | total > 30) and
//            bin.length within its 5 %..95 % quantiles; optionally thin to n.bins.reduced   -> k_rs_rowtotal + host
//   :100     per reference, Pearson correlation of length/depth-normalised counts with the test  -> k_rs_colsum,
//            k_rs_colmoments (two-pass, centred)
//   :101-102 order references by decreasing correlation                                          -> host
//   :114-115 reference_i = sum of the i best references (a prefix sum along the sorted axis)      -> k_rs_prefix
//   :117-123 new('ExomeDepth', test, reference_i): beta-binomial fit for EVERY i                 -> fit_columns
//            (the R loop is sequential; here the R fits are one batched fit with a shared test column)
//   :125-128 phi_i, mean.p_i, median(reference_i), RatioSd_i = mean(sqrt(1 + (test+reference_i-1) phi_i))
//                                                                       -> k_rs_count_le (bisection), k_rs_ratiosd
//   :130     early exit once i > 2 and mean.p < 0.05 (becomes a mask)                             -> host
//   :133-140 expected.BF_i = get.power.betabinom(round(median depth), phi, p, p_deletion)        -> k_rs_power
//   :143-145 choice = the first which.max(expected.BF) references                                -> host
// Parity: tolerance-level only.  The fits stand in for aod::betabin and the power sum for
// VGAM::dbetabinom.ab -- both third-party and not in the reference tree (parity unpinned, DESIGN.md).

namespace {

constexpr int kRsQ = kFitQ;   // quantities per partial (reuse reduce_partials)

// row totals over the R reference columns (+ the test count): one wave per bin
__global__ void __launch_bounds__(256)
k_rs_rowtotal(const int32_t* __restrict__ test, const int32_t* __restrict__ refs, int64_t E, int64_t R,
              double* __restrict__ total)
{
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= E) return;
  double acc = 0.0;
  for (int64_t r = lane; r < R; r += 64) acc += (double)refs[e * R + r];   // integers: exact in binary64
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) total[e] = acc + (double)test[e];
}

// column sums of the selected bins: partial[chunk][0][R] = sum_e refs[sel[e]][r]
__global__ void __launch_bounds__(kWave * kFitSub)
k_rs_colsum(const int32_t* __restrict__ refs, const int32_t* __restrict__ sel, int64_t n, int64_t R,
            double* __restrict__ partial)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  double s0 = 0.0;
  for (int64_t e = e0; e < e1; ++e) s0 += (double)refs[(int64_t)sel[e] * R + r];
  double* o = partial + (chunk * kRsQ) * R + r;
  o[0] = s0; o[R] = 0; o[2 * R] = 0; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
}

// finish a column reduction: out[q][r] = sum over chunks (fixed order)
__global__ void __launch_bounds__(kWave * kRedY)
k_rs_reduce(const double* __restrict__ partial, int64_t nchunk, int64_t R, double* __restrict__ out)
{
  __shared__ double lds[kRsQ][kRedY][kWave];
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool live = r < R;
  double tot[kRsQ];
  reduce_partials(partial, nchunk, R, r, live, tot, lds);
  if (!live || threadIdx.y != 0) return;
#pragma unroll
  for (int q = 0; q < kRsQ; ++q) out[q * R + r] = tot[q];
}

// normalised counts as the reference forms them (R/optimize_reference_set.R:100):
//   u = x / (bin.length * sum(x) / 10^6)
__device__ __forceinline__ double rs_norm(double x, double len, double colsum) { return x / (len * colsum / 1e6); }

// pass mode 0: sums of u (per reference) ; mode 1: centred second moments  sum (u-mu)^2, sum (u-mu)(w-mw)
//   w = normalised test counts; wsum/wmean/colmean supplied by the host between the passes
__global__ void __launch_bounds__(kWave * kFitSub)
k_rs_colmoments(const int32_t* __restrict__ refs, const int32_t* __restrict__ test, const double* __restrict__ len,
                const int32_t* __restrict__ sel, int64_t n, int64_t R, const double* __restrict__ colsum,
                double testsum, int mode, const double* __restrict__ colmean, double testmean,
                double* __restrict__ partial)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const double cs = colsum[r];
  const double mu = mode ? colmean[r] : 0.0;
  double a0 = 0, a1 = 0, a2 = 0;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t row = sel[e];
    const double L = len ? len[row] : 1.0;
    const double u = rs_norm((double)refs[row * R + r], L, cs);
    if (mode == 0) {
      a0 += u;
    } else {
      const double w = rs_norm((double)test[row], L, testsum);
      const double du = u - mu, dw = w - testmean;
      a0 += du * du; a1 += du * dw; a2 += dw * dw;
    }
  }
  double* o = partial + (chunk * kRsQ) * R + r;
  o[0] = a0; o[R] = a1; o[2 * R] = a2; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
}

// cumulative reference counts along the sorted reference axis: cum[e][i] = sum_{k<=i} refs[sel[e]][order[k]],
// kept for the prefix window [pb, pe) (the whole axis on one GPU; a contiguous share of it per rank otherwise)
// one wave per selected bin; 64 references per step, wave prefix sum + carry; coalesced stores
__global__ void __launch_bounds__(256)
k_rs_prefix(const int32_t* __restrict__ refs, const int32_t* __restrict__ sel, const int32_t* __restrict__ order,
            int64_t n, int64_t R, int64_t pb, int64_t pe, int32_t* __restrict__ cum)
{
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= n) return;
  const int32_t* __restrict__ row = refs + (int64_t)sel[e] * R;
  int32_t carry = 0;
  for (int64_t base = 0; base < pe; base += 64) {   // only prefixes pb <= i < pe are stored: cum[e][i - pb]
    const int64_t i = base + lane;
    int32_t x = (i < pe) ? row[order[i]] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t t = __shfl_up(x, d, 64);
      if (lane >= d) x += t;
    }
    if (i >= pb && i < pe) cum[e * (pe - pb) + (i - pb)] = carry + x;
    carry += __shfl(x, 63, 64);
  }
}

// median by bisection on the value: counts of cum[.][i] <= mid[i] for two targets per column
__global__ void __launch_bounds__(kWave * kFitSub)
k_rs_count_le(const int32_t* __restrict__ cum, int64_t n, int64_t R, const int32_t* __restrict__ mid0,
              const int32_t* __restrict__ mid1, double* __restrict__ partial)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const int32_t m0 = mid0[r], m1 = mid1[r];
  int c0 = 0, c1 = 0;
  for (int64_t e = e0; e < e1; ++e) {
    const int32_t x = cum[e * R + r];
    c0 += (x <= m0); c1 += (x <= m1);
  }
  double* o = partial + (chunk * kRsQ) * R + r;
  o[0] = (double)c0; o[R] = (double)c1; o[2 * R] = 0; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
}

// bisection step for both order statistics (k0-th and k1-th smallest, 0-based): smallest v with count(x <= v) > k
__global__ void k_rs_bisect(const double* __restrict__ counts, int64_t R, int64_t k0, int64_t k1, int32_t* __restrict__ lo0,
                            int32_t* __restrict__ hi0, int32_t* __restrict__ mid0, int32_t* __restrict__ lo1,
                            int32_t* __restrict__ hi1, int32_t* __restrict__ mid1)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (lo0[r] < hi0[r]) {
    if (counts[r] > (double)k0) hi0[r] = mid0[r]; else lo0[r] = mid0[r] + 1;
  }
  if (lo1[r] < hi1[r]) {
    if (counts[R + r] > (double)k1) hi1[r] = mid1[r]; else lo1[r] = mid1[r] + 1;
  }
  mid0[r] = lo0[r] + (hi0[r] - lo0[r]) / 2;
  mid1[r] = lo1[r] + (hi1[r] - lo1[r]) / 2;
}

// (edbins.inc, later in this translation unit)
__global__ void k_bins_colmax(const int32_t* __restrict__ ref, int64_t E, int64_t S, int32_t* __restrict__ pmax, const int* __restrict__ skip_from, int64_t T);
__global__ void k_bins_max_reduce(const int32_t* __restrict__ pmax, int64_t nchunk, int64_t S, int32_t* __restrict__ xmax);
__global__ void k_bins_bisect_init(const int32_t* __restrict__ xmax, int64_t S, int32_t* __restrict__ lo0, int32_t* __restrict__ hi0,
                                   int32_t* __restrict__ mid0, int32_t* __restrict__ lo1, int32_t* __restrict__ hi1,
                                   int32_t* __restrict__ mid1);
// brackets of the prefixes a cohort's batched fit skipped (k_fit_skip_prefixes) closed before the search starts: their columns cost nothing
__global__ void k_rc_close_skipped(const int* __restrict__ skip_from, int K, int64_t T, int32_t* __restrict__ lo, int32_t* __restrict__ hi);

// Medians of the K x T cumulative columns by search on the value.  Invariant: the k-th smallest value (0-based) lies in [lo, hi].
// (The single-test entry's k_rs_count_le / k_rs_bisect take one bit per pass for each of the two order statistics; round 3's cohort form
// took two bits per pass with three thresholds.)
// Four bits per pass (round 5): fifteen thresholds split the bracket in sixteen, the per-sub-chunk counts (<= 256 rows) travel as
// 16-bit words in the same partial buffer, and ONE kernel per pass sums them over the chunks and moves the bracket -- 6 passes over the
// 1.3-GB matrix of cumulative references where the two-bit form took 9-10 (each pass is the matrix read once: 0.33 ms).
constexpr int kRcT = 15;
__device__ __forceinline__ int32_t rc_threshold16(int32_t lo, int32_t hi, int j)      // j = 1 .. 15
{
  return (int32_t)((int64_t)lo + (((int64_t)hi - (int64_t)lo) * j) / 16);
}
__global__ void __launch_bounds__(kWave * kFitSub)
k_rc_count_le15(const int32_t* __restrict__ cum, int64_t n, int64_t R, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                unsigned short* __restrict__ partial /* [nchunk][16][R] */)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const int32_t l = lo[r], h = hi[r];
  if (l >= h) return;            // found (or skipped): k_rc_hex does not read this column's counts
  int32_t m[kRcT];
  int c[kRcT];
#pragma unroll
  for (int j = 0; j < kRcT; ++j) { m[j] = rc_threshold16(l, h, j + 1); c[j] = 0; }
  // eight rows requested before any is consumed (a row at a time, the loop waited out a memory round trip per row: these column passes
  // were bound by latency, not by bytes)
  int64_t e = e0;
  for (; e + 8 <= e1; e += 8) {
    int32_t x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = cum[(e + u) * R + r];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int j = 0; j < kRcT; ++j) c[j] += (x[u] <= m[j]);
    }
  }
  for (; e < e1; ++e) {
    const int32_t x = cum[e * R + r];
#pragma unroll
    for (int j = 0; j < kRcT; ++j) c[j] += (x <= m[j]);
  }
  unsigned short* o = partial + (chunk * 16) * R + r;
#pragma unroll
  for (int j = 0; j < kRcT; ++j) o[(int64_t)j * R] = (unsigned short)c[j];
}
__global__ void k_rc_hex(const unsigned short* __restrict__ partial, int64_t nchunk, int64_t R, int64_t k, int32_t* __restrict__ lo, int32_t* __restrict__ hi)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int32_t l = lo[r], h = hi[r];
  if (l >= h) return;
  int64_t c[kRcT];
#pragma unroll
  for (int j = 0; j < kRcT; ++j) c[j] = 0;
  for (int64_t ch = 0; ch < nchunk; ++ch) {
#pragma unroll
    for (int j = 0; j < kRcT; ++j) c[j] += partial[(ch * 16 + j) * R + r];
  }
  int32_t nl = l, nh = h;
  bool found = false;
#pragma unroll
  for (int j = 0; j < kRcT; ++j) {
    if (!found) {
      const int32_t mj = rc_threshold16(l, h, j + 1);
      if (c[j] > k) { nh = mj; found = true; }
      else nl = mj + 1;
    }
  }
  lo[r] = nl; hi[r] = nh;
}
// the next order statistic: v1 = v0 if more than k1 values are <= v0, else the smallest value above v0
__global__ void __launch_bounds__(kWave * kFitSub)
k_rc_next(const int32_t* __restrict__ cum, int64_t n, int64_t R, const int32_t* __restrict__ v0, double* __restrict__ partial,
          const int* __restrict__ skip_from, int64_t T)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  if (skip_from && (int)(r / T) >= skip_from[r % T]) {      // a column nobody looks at (see k_rc_close_skipped): no pass over it
    partial[(chunk * 2) * R + r] = 0.0; partial[(chunk * 2 + 1) * R + r] = 0.0;
    return;
  }
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const int32_t v = v0[r];
  int c = 0; int32_t mn = 2147483647;
  int64_t e = e0;
  for (; e + 8 <= e1; e += 8) {
    int32_t x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = cum[(e + u) * R + r];
#pragma unroll
    for (int u = 0; u < 8; ++u) { c += (x[u] <= v); mn = (x[u] > v && x[u] < mn) ? x[u] : mn; }
  }
  for (; e < e1; ++e) {
    const int32_t x = cum[e * R + r];
    c += (x <= v);
    mn = (x > v && x < mn) ? x : mn;
  }
  partial[(chunk * 2) * R + r] = (double)c;
  partial[(chunk * 2 + 1) * R + r] = (double)mn;
}
__global__ void k_rc_next_finish(const double* __restrict__ partial, int64_t nchunk, int64_t R, int64_t k1, const int32_t* __restrict__ v0,
                                 int32_t* __restrict__ v1)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  double c = 0.0, mn = 2147483647.0;
  for (int64_t ch = 0; ch < nchunk; ++ch) { c += partial[(ch * 2) * R + r]; mn = fmin(mn, partial[(ch * 2 + 1) * R + r]); }
  v1[r] = (c > (double)k1) ? v0[r] : (int32_t)mn;
}

// RatioSd numerator: sum_e sqrt(1 + (test + reference_i - 1) * phi_i)   (R/optimize_reference_set.R:128)
__global__ void __launch_bounds__(kWave * kFitSub)
k_rs_ratiosd(const int32_t* __restrict__ cum, const int32_t* __restrict__ test_sel, int64_t n, int64_t R,
             const double* __restrict__ phi, double* __restrict__ partial)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const double ph = phi[r];
  double a0 = 0.0;
  for (int64_t e = e0; e < e1; ++e)
    a0 += __builtin_sqrt(1.0 + ((double)test_sel[e] + (double)cum[e * R + r] - 1.0) * ph);
  double* o = partial + (chunk * kRsQ) * R + r;
  o[0] = a0; o[R] = 0; o[2 * R] = 0; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
}

// get.power.betabinom (R/tools.R:128-166, theory = FALSE, limit = FALSE):
//   sum_{x=0}^{size} dbetabinom.ab(x, size, alt.a, alt.b) * log10(e) * [log dbb(alt) - log dbb(null)]
//   log dbb(x; size, a, b) = lchoose(size, x) + lbeta(a + x, b + size - x) - lbeta(a, b)
//   lchoose(n, k) = -log(n + 1) - lbeta(n - k + 1, k + 1)
// grid: (x tiles, reference i); per-block sums land in partial[i][tile]; a second kernel adds them in order.
constexpr int kPowBlock = 256;
constexpr int kPowPer = 2;   // x values per thread (round 5: 8 -> 2 -- a block of 2 048 values for columns whose size is a few hundred left most lanes idle)
__global__ void __launch_bounds__(kPowBlock)
k_rs_power(const double* __restrict__ phi, const double* __restrict__ pbar, const double* __restrict__ size_d,
           const int* __restrict__ active, int64_t R, int64_t ntile, double* __restrict__ partial,
           const double* __restrict__ alt_p /* NULL: the deletion alternative of select.reference.set */,
           int theory = 0 /* 1: the binomial case of get.power.betabinom (R/tools.R:137-142): dbinom instead of dbetabinom.ab;
                             2: the `limit` case (:145-153): log ratio of the BETA densities at x / size, weighted by dbetabinom.ab(alt) */)
{
  __shared__ double red[kPowBlock];
  __shared__ double s_lb[2];
  const int64_t i = blockIdx.y;
  const int tid = threadIdx.x;
  double acc = 0.0;
  // (a block beyond the column's size has nothing to add: it leaves before the column's constants are formed)
  const bool has_work = active[i] && (double)((int64_t)blockIdx.x * kPowPer * kPowBlock) <= size_d[i];
  if (has_work) {
    const double ph = phi[i], p = pbar[i];
    const double size = size_d[i];
    const double alt_odds = p / (1 - p) * 0.5;                 // R/optimize_reference_set.R:133-134
    const double ap = alt_p ? alt_p[i] : alt_odds / (1 + alt_odds);
    const double a = p * (1 - ph) / ph, b = (1 - p) * (1 - ph) / ph;
    const double aa = ap * (1 - ph) / ph, ab = (1 - ap) * (1 - ph) / ph;
    int flag = 0;
    // the two constants of the column once per block (two threads), not once per thread
    if (theory != 1 && tid < 2) s_lb[tid] = (tid == 0) ? edsf::lnbeta(a, b, &flag) : edsf::lnbeta(aa, ab, &flag);
    __syncthreads();
    const double lb0 = (theory == 1) ? 0.0 : s_lb[0], lba0 = (theory == 1) ? 0.0 : s_lb[1];
    const double lnp1 = ed_plog(size + 1.0);
    // binomial case: log dbinom(x; size, q) = lchoose(size, x) + x log q + (size - x) log(1 - q)
    const double lap = ed_plog(ap), laq = ed_plog(1.0 - ap), lp = ed_plog(p), lq = ed_plog(1.0 - p);
    for (int k = 0; k < kPowPer; ++k) {
      const double x = (double)(((int64_t)blockIdx.x * kPowPer + k) * kPowBlock + tid);
      if (x <= size) {
        const double lch = -lnp1 - edsf::lnbeta(size - x + 1.0, x + 1.0, &flag);
        const double la = (theory == 1) ? (x * lap + (size - x) * laq) : (edsf::lnbeta(aa + x, ab + size - x, &flag) - lba0);
        const double l0 = (theory == 1) ? (x * lp + (size - x) * lq) : (edsf::lnbeta(a + x, b + size - x, &flag) - lb0);
        const double pr = ed_pexp(lch + la);
        if (theory == 2) {
          // dbeta(u; s1, s2, log = TRUE) = (s1 - 1) log u + (s2 - 1) log(1 - u) - lbeta(s1, s2) at u = x / size; the end points u = 0, 1
          // (where the densities are 0 or infinite) carry no weight worth the name and are left out
          if (x > 0.0 && x < size) {
            const double u = x / size, lu = ed_plog(u), l1u = ed_plog(1.0 - u);
            const double da = ((aa - 1.0) * lu + (ab - 1.0) * l1u) - lba0, d0 = ((a - 1.0) * lu + (b - 1.0) * l1u) - lb0;
            acc += pr * (0.43429448190325182765 * (da - d0));
          }
        } else
        acc += pr * (0.43429448190325182765 * (la - l0));      // log10(exp(1)) * BF
      }
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = kPowBlock / 2; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) partial[i * ntile + blockIdx.x] = red[0];
}

// The default case (theory = 0) by WALKING the two mass functions instead of evaluating every term from scratch (round 6: the term-by-term kernel
// above was 1.5 ms of the cohort entry's 14 -- three lnbeta per x, ~1 500 instructions).  With L(x) = log dbb(x; size, alt) and D(x) = L(x) - log
// dbb(x; size, null):
//   L(x + 1) - L(x) = log[(size - x)(aa + x) / ((x + 1)(ab + size - x - 1))]          D(x + 1) - D(x) = log[(aa + x)(b + size - x - 1) / ((a + x)(ab + size - x - 1))]
//   L(0) = lbeta(aa, ab + size) - lbeta(aa, ab) = sum_{k < size} log[(ab + k) / (aa + ab + k)]                                       (null: a, b)
// A wave owns a column.  Pass 1 sums the logarithms of L(0) (ratios multiplied four at a time, one logarithm per product); pass 2 walks x in tiles of
// 64 lanes x 4 values: a lane multiplies its four step ratios, one logarithm per lane and a wave scan place the lane on the walk, exp once per lane, the
// mass inside the lane by products and D by one logarithm per x.  One reciprocal, ~1.25 logarithms and 0.25 exp per x.  Accuracy: every step ratio is
// formed to ~3 ulp and the walk adds size / 256 + 6 rounded sums: a relative error of order 1e-15 x log2(size) in the masses -- below the 1e-13 x |lnbeta|
// the differences of lnbeta values near 1e4 carry in the term-by-term form (both are compared with the checker at 1e-9).  Sums in a fixed order.
constexpr int kPwP = 4;
__device__ __forceinline__ double pw_wave_sum(double v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ double pw_wave_scan(double v, int lane)      // inclusive
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const double o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
  return v;
}
__global__ void __launch_bounds__(256)
k_rs_power_walk(const double* __restrict__ phi, const double* __restrict__ pbar, const double* __restrict__ size_d, const int* __restrict__ active,
                int64_t R, double* __restrict__ out, const double* __restrict__ alt_p /* NULL: the deletion alternative of select.reference.set */)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= R) return;
  if (!active[i]) { if (lane == 0) out[i] = ed_pm_nan(); return; }
  const double ph = phi[i], p = pbar[i], size = size_d[i];
  const double alt_odds = p / (1 - p) * 0.5;                 // R/optimize_reference_set.R:133-134
  const double ap = alt_p ? alt_p[i] : alt_odds / (1 + alt_odds);
  const double a = p * (1 - ph) / ph, b = (1 - p) * (1 - ph) / ph;
  const double aa = ap * (1 - ph) / ph, ab = (1 - ap) * (1 - ph) / ph;
  const double tha = aa + ab, thn = a + b;
  const int64_t n = (int64_t)size;
  // pass 1: L_alt(0), L_null(0)
  double s_alt = 0.0, s_null = 0.0;
  for (int64_t k0 = (int64_t)lane * kPwP; k0 < n; k0 += 64 * kPwP) {
    double qa = 1.0, qn = 1.0;
#pragma unroll
    for (int j = 0; j < kPwP; ++j) {
      const double kd = (double)(k0 + j);
      if (k0 + j < n) {
        const double inv = edfit::frcp((tha + kd) * (thn + kd));
        qa *= (ab + kd) * (thn + kd) * inv;
        qn *= (b + kd) * (tha + kd) * inv;
      }
    }
    s_alt += edfit::flog(qa);
    s_null += edfit::flog(qn);
  }
  double carry_l = pw_wave_sum(s_alt);
  double carry_d = carry_l - pw_wave_sum(s_null);
  // pass 2: the walk
  double acc = 0.0;
  for (int64_t x0 = 0; x0 <= n; x0 += 64 * kPwP) {
    const int64_t xs = x0 + (int64_t)lane * kPwP;
    double ql[kPwP + 1], qd[kPwP + 1];       // products of the step ratios before value j of the lane
    ql[0] = 1.0; qd[0] = 1.0;
#pragma unroll
    for (int j = 0; j < kPwP; ++j) {
      double rl = 1.0, rd = 1.0;
      if (xs + j < n) {
        const double xd = (double)(xs + j);
        const double u = aa + xd, v = ab + (size - xd - 1.0), w = a + xd, t = b + (size - xd - 1.0), x1 = xd + 1.0;
        const double inv = edfit::frcp(x1 * v * w);
        rl = ((size - xd) * u) * w * inv;
        rd = (u * t) * x1 * inv;
      }
      ql[j + 1] = ql[j] * rl;
      qd[j + 1] = qd[j] * rd;
    }
    const double ll = edfit::flog(ql[kPwP]), ld = edfit::flog(qd[kPwP]);
    const double il = pw_wave_scan(ll, lane), id = pw_wave_scan(ld, lane);
    const double el = __shfl_up(il, 1, 64), ed = __shfl_up(id, 1, 64);           // the lanes before this one
    const double base_l = lane ? carry_l + el : carry_l, base_d = lane ? carry_d + ed : carry_d;
    const double pr0 = ed_pexp(base_l);
#pragma unroll
    for (int j = 0; j < kPwP; ++j)
      if (xs + j <= n) {
        const double dj = (j == 0) ? base_d : base_d + edfit::flog(qd[j]);
        acc = __builtin_fma(pr0 * ql[j], dj, acc);
      }
    carry_l += __shfl(il, 63, 64);
    carry_d += __shfl(id, 63, 64);
  }
  acc = pw_wave_sum(acc);
  if (lane == 0) out[i] = 0.43429448190325182765 * acc;      // log10(exp(1)) * BF
}

__global__ void k_rs_power_sum(const double* __restrict__ partial, int64_t R, int64_t ntile, const int* __restrict__ active,
                               double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  double s = 0.0;
  for (int64_t t = 0; t < ntile; ++t) s += partial[i * ntile + t];
  out[i] = active[i] ? s : ed_pm_nan();
}

// R's quantile(x, p), type 7: v[lo] + (h - floor(h)) (v[lo + 1] - v[lo]), h = (n - 1) p, on the order statistics of x --
// from an UNSORTED vector (reordered in place): the two order statistics by selection, O(n) instead of a sort
// (two sorts of 200 000 doubles were 15 of the 18 ms the cohort entry's bin selection took)
double r_quantile_select(std::vector<double>& v, double p)
{
  const size_t n = v.size();
  if (n == 0) return std::nan("");
  const double h = (double)(n - 1) * p;
  const double fl = std::floor(h);
  const size_t lo = (size_t)fl;
  if (lo + 1 >= n) return *std::max_element(v.begin(), v.end());
  std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)lo, v.end());
  const double a = v[lo];
  const double b = *std::min_element(v.begin() + (std::ptrdiff_t)lo + 1, v.end());   // the next order statistic
  return a + (h - fl) * (b - a);
}

// The same quantile by ONE counting pass: for non-negative doubles the bit pattern orders like the value, so a histogram of its top
// 16 bits (sign, exponent, four mantissa bits: values within a factor of two fall into 16 buckets) finds the bucket of the wanted order
// statistic, and only that bucket (~n / 20 values) is selected in.  Exact -- the two order statistics are the same numbers; 0.2 ms where
// nth_element over 200 000 doubles took 1.0-1.2 ms of the cohort entry's bin selection, three times over.  Negative values or NaN: the
// general routine.
double r_quantile_select_fast(const std::vector<double>& v, double p)
{
  const size_t n = v.size();
  auto general = [&]() { std::vector<double> c(v); return r_quantile_select(c, p); };
  if (n < 4096) return general();
  auto key = [](double x) { uint64_t k; std::memcpy(&k, &x, 8); return k; };
  std::vector<uint32_t> hist(65536, 0);
  double mx = 0.0;
  for (double x : v) {
    if (!(x >= 0.0)) return general();        // (negative or NaN)
    ++hist[key(x) >> 48];
    mx = std::max(mx, x);
  }
  const double h = (double)(n - 1) * p;
  const double fl = std::floor(h);
  const size_t lo = (size_t)fl;
  if (lo + 1 >= n) return mx;
  size_t before = 0;
  uint32_t B = 0;
  for (; B < 65536u; ++B) { if (before + hist[B] > lo) break; before += hist[B]; }
  std::vector<double> w;
  w.reserve(hist[B]);
  double min_above = std::numeric_limits<double>::infinity();
  for (double x : v) {
    const uint32_t b = (uint32_t)(key(x) >> 48);
    if (b == B) w.push_back(x);
    else if (b > B && x < min_above) min_above = x;
  }
  const size_t k = lo - before;
  std::nth_element(w.begin(), w.begin() + (std::ptrdiff_t)k, w.end());
  const double a = w[k];
  const double b = (k + 1 < w.size()) ? *std::min_element(w.begin() + (std::ptrdiff_t)k + 1, w.end()) : min_above;
  return a + (h - fl) * (b - a);
}

// R's round(): IEC 60559 half-to-even on x.5 (R >= 4.0.0)
double r_round(double x) { return std::nearbyint(x); }

}  // namespace

// The two order statistics k0 <= k1 <= k0 + 1 (0-based) of every column of cum[n][R] -- the median's two halves -- into lo0 = di32[0..R)
// and lo1 = di32[3R..4R): brackets [0, column maximum], two bits per pass, then the next order statistic in one more pass.
// d_skip (optional, cohort entry): per test the first prefix whose column is not needed (column = prefix * T + test).
static int refset_medians(const int32_t* cum, int64_t n, int64_t R, int64_t k0, int64_t k1, int32_t* di32, double* dpart, double* dred,
                          int32_t* dpmax, int32_t* dxmax, const int* d_skip, int K, int64_t T, hipStream_t st)
{
  const int64_t nblk = (n + kFitChunk - 1) / kFitChunk, nchunk = nblk * kFitSub;
  const dim3 gcolw((unsigned)((R + kWave - 1) / kWave), (unsigned)nblk), bcol(kWave, kFitSub), gredw((unsigned)((R + kWave - 1) / kWave)), bred(kWave, kRedY);
  const dim3 g1((unsigned)((R + 255) / 256)), b1(256);
  int32_t* lo0 = di32; int32_t* hi0 = lo0 + R; int32_t* mid0 = hi0 + R;
  int32_t* lo1 = mid0 + R; int32_t* hi1 = lo1 + R; int32_t* mid1 = hi1 + R;
  hipLaunchKernelGGL(k_bins_colmax, gcolw, bcol, 0, st, cum, n, R, dpmax, d_skip, d_skip ? T : (int64_t)1);
  hipLaunchKernelGGL(k_bins_max_reduce, g1, b1, 0, st, dpmax, nchunk, R, dxmax);
  hipLaunchKernelGGL(k_bins_bisect_init, g1, b1, 0, st, dxmax, R, lo0, hi0, mid0, lo1, hi1, mid1);
  if (d_skip) hipLaunchKernelGGL(k_rc_close_skipped, g1, b1, 0, st, d_skip, K, T, lo0, hi0);
  std::vector<int32_t> hx((size_t)R);
  HIP_TRY(hipMemcpyAsync(hx.data(), dxmax, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int32_t gmax = 0;
  for (int32_t v : hx) gmax = std::max(gmax, v);
  int bits = 1;
  while ((int64_t)1 << bits <= (int64_t)gmax) ++bits;
  // (the partial buffer holds nchunk x kRsQ doubles per column = 48 bytes: room for the 16 x 2 bytes of a pass)
  static_assert(kRsQ * 8 >= 32, "partial buffer too small for the 16-bit counts");
  const int passes = (bits + 3) / 4 + 1;
  for (int it = 0; it < passes; ++it) {
    hipLaunchKernelGGL(k_rc_count_le15, gcolw, bcol, 0, st, cum, n, R, lo0, hi0, reinterpret_cast<unsigned short*>(dpart));
    hipLaunchKernelGGL(k_rc_hex, g1, b1, 0, st, reinterpret_cast<const unsigned short*>(dpart), nchunk, R, k0, lo0, hi0);
  }
  if (k1 == k0) HIP_TRY(hipMemcpyAsync(lo1, lo0, (size_t)R * 4, hipMemcpyDeviceToDevice, st));
  else {
    hipLaunchKernelGGL(k_rc_next, gcolw, bcol, 0, st, cum, n, R, lo0, dpart, d_skip, d_skip ? T : (int64_t)1);
    hipLaunchKernelGGL(k_rc_next_finish, g1, b1, 0, st, dpart, nchunk, R, k1, lo0, lo1);
  }
  HIP_TRY(hipGetLastError());
  return ED_OK;
}

// 0-based positions picked by  x[seq(1, len, len / n_reduced)]  (R/optimize_reference_set.R:86).  R's seq.default with a
// fractional `by`:  n <- as.integer((to - from) / by + 1e-10);  from + (0:n) * by, clipped with pmin(., to); a fractional
// subscript truncates.  (Positions are products k * by, NOT repeated additions: the two differ in the last bit often
// enough to pick a different bin for about a quarter of the (len, n_reduced) pairs.)  Host code only.
ED_EXPORT int ed_refset_thin_positions(int64_t len, int64_t n_reduced, int64_t* positions, int64_t cap, int64_t* n_positions)
try {
  if (len < 1 || n_reduced < 1 || !n_positions || cap < 0 || (cap > 0 && !positions))
    return ed_fail(ED_ERR_INVALID, "ed_refset_thin_positions: bad arguments");
  const double by = (double)len / (double)n_reduced;
  const int64_t nn = (int64_t)(((double)len - 1.0) / by + 1e-10);
  int64_t k = 0;
  for (; k <= nn; ++k) {
    const double pos = std::fmin(1.0 + (double)k * by, (double)len);
    if (k < cap) positions[k] = (int64_t)pos - 1;
  }
  *n_positions = k;
  return ED_OK;
}
ED_CATCH("ed_refset_thin_positions")

// Bin selection of select.reference.set (R/optimize_reference_set.R:79-88): bins with total > 30, total below the 90 % quantile
// of those totals, bin.length within its 5 % .. 95 % quantiles; optionally thinned to n.bins.reduced (R's seq()).  `total` is
// rowSums(reference.counts) + test.counts -- for a cohort in which every other sample is a candidate, the same for every test.
// The 5 % / 95 % quantiles of the bin lengths (R/optimize_reference_set.R:82-83) depend on nothing the device computes: a caller that
// starts them on host threads BEFORE it launches the row totals (LengthQuantiles::start) finds them ready when the totals arrive.
struct LengthQuantiles {
  double l05 = 1.0, l95 = 1.0;
  bool failed = false;            // the thread ran out of host memory (nothing may leave a thread's function): the caller reports it after join()
  std::thread t05;
  void start(const double* bin_length, int64_t E)
  {
    if (!bin_length) return;
    t05 = std::thread([this, bin_length, E]() {
      try { std::vector<double> ls(bin_length, bin_length + E); l05 = r_quantile_select_fast(ls, 0.05); l95 = r_quantile_select_fast(ls, 0.95); }
      catch (...) { failed = true; }
    });
  }
  void join() { if (t05.joinable()) t05.join(); }
  ~LengthQuantiles() { join(); }
};

static int refset_select_bins(const std::vector<double>& total, const double* bin_length, int64_t E, int64_t n_bins_reduced,
                              std::vector<int32_t>& sel, LengthQuantiles* lq = nullptr)
{
  std::vector<double> big;
  big.reserve((size_t)E);
  for (int64_t e = 0; e < E; ++e) if (total[e] > 30) big.push_back(total[e]);
  double q90 = 0, l05 = 1, l95 = 1;
  {
    LengthQuantiles own;
    if (!lq) { own.start(bin_length, E); lq = &own; }
    q90 = r_quantile_select_fast(big, 0.9);
    lq->join();
    if (lq->failed) return ed_fail(ED_ERR_NOMEM, "select.reference.set: out of host memory (bin-length quantiles)");
    l05 = lq->l05; l95 = lq->l95;
  }
  sel.clear();
  sel.reserve((size_t)E);
  for (int64_t e = 0; e < E; ++e) {
    const double L = bin_length ? bin_length[e] : 1.0;
    if (total[e] > 30 && L >= l05 && L <= l95 && total[e] < q90) sel.push_back((int32_t)e);
  }
  if (n_bins_reduced > 0 && n_bins_reduced < (int64_t)sel.size()) {
    // selected[seq(1, length(selected), length(selected) / n.bins.reduced)]  (R/optimize_reference_set.R:86)
    std::vector<int64_t> pos((size_t)n_bins_reduced + 2);
    int64_t np = 0;
    if (int rc = ed_refset_thin_positions((int64_t)sel.size(), n_bins_reduced, pos.data(), (int64_t)pos.size(), &np)) return rc;
    std::vector<int32_t> thin;
    for (int64_t k = 0; k < np; ++k) thin.push_back(sel[(size_t)pos[k]]);
    sel.swap(thin);
  }
  return ED_OK;
}

// R/optimize_reference_set.R:104-111, :130, :143-145 on a complete table of per-prefix statistics: the loop's
// early exit (statistics recorded up to and including the iteration that breaks, expected.BF only before it)
// and reference.choice = the first which.max(expected.BF) references.  Host code only.
ED_EXPORT int ed_refset_finalize(ed_refset_row* rows, int64_t n_refs, int32_t* n_chosen)
try {
  if (!rows || !n_chosen || n_refs <= 0) return ed_fail(ED_ERR_INVALID, "ed_refset_finalize: bad arguments");
  bool stopped = false, seen_stop = false;
  int64_t best = -1;
  const double na = std::nan("");
  for (int64_t i = 0; i < n_refs; ++i) {
    ed_refset_row& o = rows[i];
    o.selected = 0;
    if (!stopped && i + 1 > 2 && o.mean_p < 0.05) stopped = true;
    const bool active = !stopped;
    const bool recorded = !seen_stop;   // the iteration that triggers the break still records its statistics
    if (!active) seen_stop = true;
    if (!recorded) o.phi = o.mean_p = o.median_depth = o.ratio_sd = na;
    if (!active) o.expected_BF = na;
    if (active && !std::isnan(o.expected_BF) && (best < 0 || o.expected_BF > rows[best].expected_BF)) best = i;
  }
  if (best < 0) return ed_fail(ED_ERR_STATE, "ed_select_reference_set: no finite expected Bayes factor");
  rows[best].selected = 1;
  *n_chosen = (int32_t)(best + 1);
  return ED_OK;
}
ED_CATCH("ed_refset_finalize")

// The statistics of the cumulative references i in [prefix_begin, prefix_end) of the correlation-sorted axis;
// every row gets ref_index and correlation.  The prefixes are independent given the sorted order, so N ranks that
// each hold the count matrix take contiguous shares of them and exchange nothing but the rows
// (exomedepth_amd/dist.py::select_reference_set_sharded); the whole axis + ed_refset_finalize is
// ed_select_reference_set.
// `clip`: for the whole axis, only the prefixes up to where the reference's loop is expected to break are formed and evaluated
// (the proportion falls as references are added; its estimate from the column sums below 0.04 -- 20 % of margin under the loop's
// 0.05 -- marks the last prefix needed): at 2048 candidates the loop breaks after ~20 of them and the other 2027 prefixes were
// 99 % of the work.  *clipped_short = the fitted loop did not break inside the clipped window (never seen): the caller repeats
// the call unclipped.  A share of the axis (ed_select_reference_set_part proper) is never clipped.
static int refset_part_impl(const int32_t* d_test, const int32_t* d_refs, int64_t n_bins, int64_t n_refs,
                            const double* bin_length, int64_t n_bins_reduced, int64_t prefix_begin,
                            int64_t prefix_end, ed_refset_row* rows, int32_t* n_chosen,
                            int64_t* n_selected_bins, void* stream_, bool clip, bool* clipped_short)
{
  *clipped_short = false;
  if (!d_test || !d_refs || !rows || !n_chosen || n_bins <= 0 || n_refs <= 0)
    return ed_fail(ED_ERR_INVALID, "ed_select_reference_set: bad arguments");
  if (prefix_begin < 0 || prefix_end > n_refs || prefix_begin >= prefix_end)
    return ed_fail(ED_ERR_INVALID, "ed_select_reference_set_part: empty or out-of-range prefix window [%lld, %lld)",
                   (long long)prefix_begin, (long long)prefix_end);
  const bool whole = (prefix_begin == 0 && prefix_end == n_refs);
  const int64_t pb = prefix_begin;
  int64_t pe = prefix_end;
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const int64_t E = n_bins, R = n_refs;
  if (bin_length)
    for (int64_t e = 0; e < E; ++e)
      if (bin_length[e] == 0) return ed_fail(ED_ERR_INVALID, "bin.length contains zeros. All bin lengths must be positive");
  // ---- bin selection (R/optimize_reference_set.R:79-97) ----
  DevBuf<void> dtotal;
  HIP_TRY(dtotal.alloc((size_t)E * 8));
  hipLaunchKernelGGL(k_rs_rowtotal, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, st, d_test, d_refs, E, R, dtotal.as<double>());
  std::vector<double> total((size_t)E);
  std::vector<int32_t> test_h((size_t)E);
  HIP_TRY(hipMemcpyAsync(total.data(), dtotal.get(), (size_t)E * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(test_h.data(), d_test, (size_t)E * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int64_t n_gt2 = 0;
  for (int64_t e = 0; e < E; ++e) n_gt2 += test_h[e] > 2;
  for (int64_t i = 0; i < R; ++i) {
    rows[i].ref_index = (int32_t)i; rows[i].selected = 0;
    rows[i].correlation = rows[i].expected_BF = rows[i].phi = rows[i].ratio_sd = rows[i].mean_p = rows[i].median_depth = std::nan("");
  }
  if (n_selected_bins) *n_selected_bins = 0;
  if (n_gt2 < 5) {   // :57-61: too little coverage, return the first reference
    *n_chosen = 1;
    return ED_OK;
  }
  std::vector<int32_t> sel;
  if (int rc = refset_select_bins(total, bin_length, E, n_bins_reduced, sel)) return rc;
  const int64_t n = (int64_t)sel.size();
  if (n_selected_bins) *n_selected_bins = n;
  if (n < 2) return ed_fail(ED_ERR_STATE, "ed_select_reference_set: fewer than 2 bins selected");
  // ---- device buffers ----
  const int64_t nblk = (n + kFitChunk - 1) / kFitChunk, nchunk = nblk * kFitSub;
  DevBuf<void> dsel, dlen, dpart, dred, dcolsum, dcolmean, dorder, dcum, dtsel, dphi, dp, di32, dsize, dact, dbf;
  HIP_TRY(dsel.alloc((size_t)n * 4));
  HIP_TRY(hipMemcpyAsync(dsel.get(), sel.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (bin_length) {
    HIP_TRY(dlen.alloc((size_t)E * 8));
    HIP_TRY(hipMemcpyAsync(dlen.get(), bin_length, (size_t)E * 8, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(dpart.alloc((size_t)nchunk * kRsQ * R * 8));
  HIP_TRY(dred.alloc((size_t)kRsQ * R * 8));
  HIP_TRY(dcolsum.alloc((size_t)R * 8));
  HIP_TRY(dcolmean.alloc((size_t)R * 8));
  const dim3 gcol((unsigned)((R + kWave - 1) / kWave), (unsigned)nblk), bcol(kWave, kFitSub);
  const dim3 gred((unsigned)((R + kWave - 1) / kWave)), bred(kWave, kRedY);
  std::vector<double> red((size_t)kRsQ * R);
  auto reduce_to_host = [&](int64_t cols) -> int {   // red[q * cols + r]
    hipLaunchKernelGGL(k_rs_reduce, dim3((unsigned)((cols + kWave - 1) / kWave)), bred, 0, st, dpart.as<double>(), nchunk, cols,
                       dred.as<double>());
    HIP_TRY(hipMemcpyAsync(red.data(), dred.get(), (size_t)kRsQ * cols * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ED_OK;
  };
  // ---- correlations (R/optimize_reference_set.R:100) ----
  hipLaunchKernelGGL(k_rs_colsum, gcol, bcol, 0, st, d_refs, dsel.as<int32_t>(), n, R, dpart.as<double>());
  if (int rc = reduce_to_host(R)) return rc;
  std::vector<double> colsum(red.begin(), red.begin() + R), colmean((size_t)R), corr((size_t)R);
  HIP_TRY(hipMemcpyAsync(dcolsum.get(), colsum.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
  double testsum = 0;
  for (int64_t e = 0; e < n; ++e) testsum += (double)test_h[sel[e]];
  double testmean = 0;
  for (int64_t e = 0; e < n; ++e) {
    const double L = bin_length ? bin_length[sel[e]] : 1.0;
    testmean += (double)test_h[sel[e]] / (L * testsum / 1e6);
  }
  testmean /= (double)n;
  hipLaunchKernelGGL(k_rs_colmoments, gcol, bcol, 0, st, d_refs, d_test, bin_length ? dlen.as<double>() : nullptr,
                     dsel.as<int32_t>(), n, R, dcolsum.as<double>(), testsum, 0, (const double*)nullptr, 0.0, dpart.as<double>());
  if (int rc = reduce_to_host(R)) return rc;
  for (int64_t r = 0; r < R; ++r) colmean[r] = red[r] / (double)n;
  HIP_TRY(hipMemcpyAsync(dcolmean.get(), colmean.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_rs_colmoments, gcol, bcol, 0, st, d_refs, d_test, bin_length ? dlen.as<double>() : nullptr,
                     dsel.as<int32_t>(), n, R, dcolsum.as<double>(), testsum, 1, dcolmean.as<double>(), testmean, dpart.as<double>());
  if (int rc = reduce_to_host(R)) return rc;
  for (int64_t r = 0; r < R; ++r) corr[r] = red[R + r] / std::sqrt(red[r] * red[2 * R + r]);
  // order(my.correlations, decreasing = TRUE): stable for ties, NA (NaN) last
  std::vector<int32_t> order((size_t)R);
  for (int64_t r = 0; r < R; ++r) order[r] = (int32_t)r;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    const bool na = std::isnan(corr[a]), nb = std::isnan(corr[b]);
    if (na != nb) return nb;
    return corr[a] > corr[b]; });
  if (clip && whole) {
    double run = 0.0;
    for (int64_t i = 0; i < R; ++i) {
      run += colsum[(size_t)order[(size_t)i]];
      if (i + 1 > 2 && testsum / (testsum + run) < 0.04) { pe = i + 1; break; }
    }
  }
  // ---- cumulative references + batched fits (R/optimize_reference_set.R:114-123) ----
  const int64_t Rw = pe - pb;   // width of the prefix window: everything below is per prefix of the window
  const dim3 gcolw((unsigned)((Rw + kWave - 1) / kWave), (unsigned)nblk), gredw((unsigned)((Rw + kWave - 1) / kWave));
  HIP_TRY(dorder.alloc((size_t)R * 4));
  HIP_TRY(hipMemcpyAsync(dorder.get(), order.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(dcum.alloc((size_t)n * Rw * 4));
  hipLaunchKernelGGL(k_rs_prefix, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_refs, dsel.as<int32_t>(),
                     dorder.as<int32_t>(), n, R, pb, pe, dcum.as<int32_t>());
  std::vector<int32_t> tsel((size_t)n);
  for (int64_t e = 0; e < n; ++e) tsel[e] = test_h[sel[e]];
  HIP_TRY(dtsel.alloc((size_t)n * 4));
  HIP_TRY(hipMemcpyAsync(dtsel.get(), tsel.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(dphi.alloc((size_t)Rw * 8));
  HIP_TRY(dp.alloc((size_t)Rw * 8));
  {
    FitWork w;
    if (int rc = w.alloc(n, Rw)) return rc;
    const int rc = fit_columns(w, FitJob::shared_test(dtsel.as<int32_t>(), dcum.as<int32_t>(), Rw).over(n, Rw).into(dphi.as<double>(), dp.as<double>()), st);
    HIP_TRY(hipStreamSynchronize(st));
    if (rc) return rc;
  }
  std::vector<double> phi((size_t)Rw), pbar((size_t)Rw);
  HIP_TRY(hipMemcpy(phi.data(), dphi.get(), (size_t)Rw * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pbar.data(), dp.get(), (size_t)Rw * 8, hipMemcpyDeviceToHost));
  // ---- median(reference_i): two order statistics per column by bisection on the value ----
  const int64_t k0 = (n - 1) / 2, k1 = n / 2;
  HIP_TRY(di32.alloc((size_t)6 * Rw * 4));
  int32_t* lo0 = di32.as<int32_t>(); int32_t* hi0 = lo0 + Rw; int32_t* mid0 = hi0 + Rw;
  int32_t* lo1 = mid0 + Rw; int32_t* hi1 = lo1 + Rw; int32_t* mid1 = hi1 + Rw;
  {
    DevBuf<void> dpmax, dxmax;
    HIP_TRY(dpmax.alloc((size_t)nchunk * Rw * 4));
    HIP_TRY(dxmax.alloc((size_t)Rw * 4));
    if (int rc = refset_medians(dcum.as<int32_t>(), n, Rw, k0, k1, di32.as<int32_t>(), dpart.as<double>(), dred.as<double>(), dpmax.as<int32_t>(),
                                dxmax.as<int32_t>(), nullptr, 0, 0, st))
      return rc;
  }
  std::vector<int32_t> med((size_t)6 * Rw);
  HIP_TRY(hipMemcpyAsync(med.data(), di32.get(), med.size() * 4, hipMemcpyDeviceToHost, st));
  // ---- RatioSd ----
  hipLaunchKernelGGL(k_rs_ratiosd, gcolw, bcol, 0, st, dcum.as<int32_t>(), dtsel.as<int32_t>(), n, Rw, dphi.as<double>(),
                     dpart.as<double>());
  if (int rc = reduce_to_host(Rw)) return rc;
  std::vector<double> median((size_t)Rw), ratio_sd((size_t)Rw), size_v((size_t)Rw);
  std::vector<int> active((size_t)Rw, 1);
  bool stopped = false;
  for (int64_t i = 0; i < Rw; ++i) {
    median[i] = 0.5 * ((double)med[i] + (double)med[3 * Rw + i]);   // lo0 / lo1 after convergence
    ratio_sd[i] = red[i] / (double)n;
    size_v[i] = r_round(median[i]);
    // the Rw loop records the statistics of iteration i, then breaks before computing expected.BF (:130)
    if (whole && !stopped && i + 1 > 2 && pbar[i] < 0.05) stopped = true;   // a share computes every prefix it owns
    active[i] = stopped ? 0 : 1;
  }
  if (clip && whole && pe < R && !stopped) { *clipped_short = true; return ED_OK; }
  // ---- expected Bayes factor of every active prefix (R/optimize_reference_set.R:133-140) ----
  HIP_TRY(dsize.alloc((size_t)Rw * 8));
  HIP_TRY(dact.alloc((size_t)Rw * 4));
  HIP_TRY(dbf.alloc((size_t)Rw * 8));
  HIP_TRY(hipMemcpyAsync(dsize.get(), size_v.data(), (size_t)Rw * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dact.get(), active.data(), (size_t)Rw * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_rs_power_walk, dim3((unsigned)((Rw + 3) / 4)), dim3(256), 0, st, dphi.as<double>(), dp.as<double>(), dsize.as<double>(),
                     dact.as<int>(), Rw, dbf.as<double>(), (const double*)nullptr);
  std::vector<double> bf((size_t)Rw);
  HIP_TRY(hipMemcpyAsync(bf.data(), dbf.get(), (size_t)Rw * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  // ---- assemble: raw statistics of the window; the loop's early exit and the choice are ed_refset_finalize's ----
  for (int64_t i = 0; i < R; ++i) {
    ed_refset_row& o = rows[i];
    o.ref_index = order[i];
    o.correlation = corr[order[i]];
  }
  for (int64_t i = 0; i < Rw; ++i) {
    ed_refset_row& o = rows[pb + i];
    o.phi = phi[i]; o.mean_p = pbar[i]; o.median_depth = median[i]; o.ratio_sd = ratio_sd[i];
    o.expected_BF = active[i] ? bf[i] : std::nan("");
  }
  *n_chosen = 0;
  return ED_OK;
}

ED_EXPORT int ed_select_reference_set_part(const int32_t* d_test, const int32_t* d_refs, int64_t n_bins, int64_t n_refs,
                                           const double* bin_length, int64_t n_bins_reduced, int64_t prefix_begin,
                                           int64_t prefix_end, ed_refset_row* rows, int32_t* n_chosen,
                                           int64_t* n_selected_bins, void* stream_)
try {
  bool short_window = false;
  if (int rc = refset_part_impl(d_test, d_refs, n_bins, n_refs, bin_length, n_bins_reduced, prefix_begin, prefix_end, rows, n_chosen,
                                n_selected_bins, stream_, true, &short_window))
    return rc;
  if (!short_window) return ED_OK;
  return refset_part_impl(d_test, d_refs, n_bins, n_refs, bin_length, n_bins_reduced, prefix_begin, prefix_end, rows, n_chosen, n_selected_bins,
                          stream_, false, &short_window);
}
ED_CATCH("ed_select_reference_set_part")

ED_EXPORT int ed_select_reference_set(const int32_t* d_test, const int32_t* d_refs, int64_t n_bins, int64_t n_refs,
                                      const double* bin_length, int64_t n_bins_reduced, ed_refset_row* rows,
                                      int32_t* n_chosen, int64_t* n_selected_bins, void* stream_)
try {
  if (!n_chosen) return ed_fail(ED_ERR_INVALID, "ed_select_reference_set: bad arguments");
  int64_t nsel = -1;
  if (int rc = ed_select_reference_set_part(d_test, d_refs, n_bins, n_refs, bin_length, n_bins_reduced, 0, n_refs, rows,
                                            n_chosen, &nsel, stream_))
    return rc;
  if (n_selected_bins) *n_selected_bins = nsel;
  if (*n_chosen == 1 && nsel == 0) return ED_OK;   // too little coverage: the first reference (:57-61)
  return ed_refset_finalize(rows, n_refs, n_chosen);
}
ED_CATCH("ed_select_reference_set")


// get.power.betabinom(size, my.phi, my.p, my.alt.p) (reference R/tools.R:128-166) in its default mode (theory = FALSE,
// frequentist = FALSE, limit = FALSE): sum_{x=0}^{size} dbetabinom(x; alt) * log10 BF(x), for n parameter sets at once.
// HOST arrays.  VGAM::dbetabinom.ab is not in the reference tree: the density is lchoose + lbeta - lbeta evaluated
// with the emission kernels' log-Beta (parity unpinned, tolerance-level against oracle/refset_oracle.py).
ED_EXPORT int ed_get_power_betabinom(int64_t n, const double* size, const double* phi, const double* p, const double* alt_p,
                                     double* out)
try {
  return ed_get_power_betabinom_mode(n, size, phi, p, alt_p, 0, out);
}
ED_CATCH("ed_get_power_betabinom")

ED_EXPORT int ed_get_power_betabinom_mode(int64_t n, const double* size, const double* phi, const double* p, const double* alt_p,
                                          int theory, double* out)
try {
  if (n < 0 || (n > 0 && (!size || !phi || !p || !alt_p || !out))) return ed_fail(ED_ERR_INVALID, "ed_get_power_betabinom: bad arguments");
  if (theory < 0 || theory > 2) return ed_fail(ED_ERR_INVALID, "ed_get_power_betabinom_mode: mode 0 (default), 1 (theory) or 2 (limit)");
  if (theory == 1)
    for (int64_t i = 0; i < n; ++i)
      if (!(p[i] > 0 && p[i] < 1 && alt_p[i] > 0 && alt_p[i] < 1))
        return ed_fail(ED_ERR_INVALID, "ed_get_power_betabinom (theory): 0 < my.p, my.alt.p < 1 required (entry %lld)", (long long)i);
  if (int rc = require_device()) return rc;
  if (n == 0) return ED_OK;
  double max_size = 0;
  std::vector<int> act((size_t)n, 1);
  for (int64_t i = 0; i < n; ++i) {
    if (!(size[i] >= 0) || (theory != 1 && !(phi[i] > 0 && phi[i] < 1))) return ed_fail(ED_ERR_INVALID, "ed_get_power_betabinom: size >= 0 and 0 < phi < 1 required (entry %lld)", (long long)i);
    max_size = std::max(max_size, std::floor(size[i]));
  }
  const int64_t per_block = (int64_t)kPowBlock * kPowPer;
  const int64_t ntile = std::max<int64_t>(1, ((int64_t)max_size + 1 + per_block - 1) / per_block);
  DevBuf<void> dsize, dphi, dp, dalt, dact, dpow, dbf;
  HIP_TRY(dsize.alloc((size_t)n * 8)); HIP_TRY(dphi.alloc((size_t)n * 8)); HIP_TRY(dp.alloc((size_t)n * 8));
  HIP_TRY(dalt.alloc((size_t)n * 8)); HIP_TRY(dact.alloc((size_t)n * 4)); HIP_TRY(dpow.alloc((size_t)n * ntile * 8));
  HIP_TRY(dbf.alloc((size_t)n * 8));
  std::vector<double> fl((size_t)n);
  for (int64_t i = 0; i < n; ++i) fl[i] = std::floor(size[i]);   // 0:size
  HIP_TRY(hipMemcpy(dsize.get(), fl.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dphi.get(), phi, (size_t)n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dp.get(), p, (size_t)n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dalt.get(), alt_p, (size_t)n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dact.get(), act.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  // the default case walks the mass functions (k_rs_power_walk); parameters whose products (size x (a + b)^2) would leave binary64's range keep the
  // term-by-term form (which has long lost its digits there: differences of lnbeta values of order 1 / phi)
  bool walk = theory == 0 && max_size < 1e15;
  for (int64_t i = 0; i < n && walk; ++i) walk = phi[i] >= 1e-140 && p[i] > 1e-140 && alt_p[i] > 1e-140 && p[i] < 1 && alt_p[i] < 1;
  if (walk)
    hipLaunchKernelGGL(k_rs_power_walk, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, dphi.as<double>(), dp.as<double>(), dsize.as<double>(),
                       dact.as<int>(), n, dbf.as<double>(), dalt.as<double>());
  else {
    hipLaunchKernelGGL(k_rs_power, dim3((unsigned)ntile, (unsigned)n), dim3(kPowBlock), 0, 0, dphi.as<double>(), dp.as<double>(),
                       dsize.as<double>(), dact.as<int>(), n, ntile, dpow.as<double>(), dalt.as<double>(), theory);
    hipLaunchKernelGGL(k_rs_power_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dpow.as<double>(), n, ntile, dact.as<int>(),
                       dbf.as<double>());
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dbf.get(), (size_t)n * 8, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_get_power_betabinom_mode")
