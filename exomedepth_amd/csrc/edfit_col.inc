// edfit_col.inc -- a column's dispersion fit on the TAIL COUNTS of its three count histograms, one workgroup per column (round 6).  Included by edfit.inc
// after the kernels of the per-cell and histogram forms (it needs fit_newton_step); used by the cohort reference sets' chunk loop (edrefcohort.inc: k_rc_column, where the scheme is described).
//
//   sum_cells [psi(a + y) - psi(a)] = sum_k T_y(k) / (a + k),   T_y(k) = #cells with y > k        (psi': squares; r with b, n = y + r with a + b)
//
// so the gradient and Hessian of the beta-binomial log-likelihood in (a, b) are six sums over the occupied bins of the tail counts -- positive terms, no
// cancellation between psi values of order log(count), one reciprocal per FOUR bins -- and a Newton iteration costs ~10^4 bin visits whatever the number of cells.

namespace {

constexpr int kColOv = 1024;                             // values beyond the bins kept per coordinate (16 bits each: a value of 65 535 or more raises the flag)

// six sums over the workgroup, in a fixed order (lanes by butterfly, then the waves one after the other)
template <int NT>
__device__ __forceinline__ void col_sum6(double (&v)[6], double (*red)[NT / 64], int tid)
{
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
  __syncthreads();                                    // (the previous reduction's readers are done)
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < 6; ++q) red[q][tid >> 6] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    double t = red[q][0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t += red[q][w];
    v[q] = t;
  }
}

// bins -> tail counts, in place, over the bins that can hold a count, [0, lim): h[k] = #values > k = sum_{v > k} hist[v] + n_beyond
template <int NT, class BinT>
__device__ __forceinline__ void col_tails(BinT* __restrict__ h, int lim, uint32_t n_beyond, uint32_t* __restrict__ wtot, int tid)
{
  const int L = (lim + NT - 1) / NT;                            // a contiguous segment per thread
  const int k0 = min(tid * L, lim), k1 = min(k0 + L, lim);
  uint32_t tot = 0;
  for (int k = k0; k < k1; ++k) tot += h[k];
  // the segments after this thread's: inclusive suffix scan over the lanes, then the later waves' totals
  uint32_t inc = tot;
  const int lane = tid & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(inc, d, 64); if (lane + d < 64) inc += o; }
  __syncthreads();
  if (lane == 0) wtot[tid >> 6] = inc;
  __syncthreads();
  uint32_t after = inc - tot + n_beyond;
  for (int w = (tid >> 6) + 1; w < NT / 64; ++w) after += wtot[w];
  for (int k = k1 - 1; k >= k0; --k) { const uint32_t v = h[k]; h[k] = (BinT)after; after += v; }
  __syncthreads();
}

// sum_k T(k) / (x + k) and sum_k T(k) / (x + k)^2 over the bins [0, lim), four consecutive bins per step: ONE reciprocal (of the product of the four
// arguments) serves the four, and the 16-bit counts become binary64 through the exponent trick (2^52 | v) - 2^52 instead of a conversion -- the
// conversions and v_rcp_f64 run at a quarter of the multiply-add rate and were two thirds of the loop.  Bins in [lim, the next multiple of 4) hold 0.
__device__ __forceinline__ double col_u32_to_f64(uint32_t v) { return __builtin_bit_cast(double, 0x4330000000000000ull | (uint64_t)v) - 0x1p52; }
__device__ __forceinline__ void col_load4(const uint16_t* __restrict__ h, double (&c)[4])
{
  const uint2 w = *(const uint2*)h;
  c[0] = col_u32_to_f64(w.x & 0xffffu); c[1] = col_u32_to_f64(w.x >> 16); c[2] = col_u32_to_f64(w.y & 0xffffu); c[3] = col_u32_to_f64(w.y >> 16);
}
__device__ __forceinline__ void col_load4(const uint32_t* __restrict__ h, double (&c)[4])
{
  const uint4 w = *(const uint4*)h;
  c[0] = col_u32_to_f64(w.x); c[1] = col_u32_to_f64(w.y); c[2] = col_u32_to_f64(w.z); c[3] = col_u32_to_f64(w.w);
}
template <int NT, class BinT>
__device__ __forceinline__ void col_tail_sums(const BinT* __restrict__ h, int lim, double x, double& s1, double& s2, int tid)
{
  for (int g = tid; 4 * g < lim; g += NT) {
    double c[4];
    col_load4(h + 4 * g, c);
    const double z0 = x + (double)(4 * g), z1 = z0 + 1.0, z2 = z0 + 2.0, z3 = z0 + 3.0;
    const double p01 = z0 * z1, p23 = z2 * z3;
    const double ip = edfit::frcp(p01 * p23);
    const double i01 = p23 * ip, i23 = p01 * ip;
    const double w0 = z1 * i01, w1 = z0 * i01, w2 = z3 * i23, w3 = z2 * i23;
    s1 = __builtin_fma(c[0], w0, s1); s2 = __builtin_fma(c[0] * w0, w0, s2);
    s1 = __builtin_fma(c[1], w1, s1); s2 = __builtin_fma(c[1] * w1, w1, s2);
    s1 = __builtin_fma(c[2], w2, s1); s2 = __builtin_fma(c[2] * w2, w2, s2);
    s1 = __builtin_fma(c[3], w3, s1); s2 = __builtin_fma(c[3] * w3, w3, s2);
  }
}

// ascending bitonic sort of kColOv 16-bit values in LDS (unused slots hold 0xffff)
template <int NT>
__device__ __forceinline__ void col_sort(uint16_t* __restrict__ a, int tid)
{
  for (int k = 2; k <= kColOv; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < kColOv; t += NT) {
        const int x = t ^ j;
        if (x > t) {
          const uint16_t u = a[t], w = a[x];
          const bool up = (t & k) == 0;
          if ((u > w) == up) { a[t] = w; a[x] = u; }
        }
      }
    }
  __syncthreads();
}


// (Round 6 also built the samples' own fit of a sample-major slab this way -- one 1 024-thread workgroup per sample, 4 096 / 16 384 / 16 384 32-bit bins, the CU's
// whole LDS -- and took it out again: 1.1-1.3 ms per 1 024 samples x 200 000 exons against 0.34 + 0.6 (depth 100) to 0.57 + 0.83 ms (aggregate references) for
// k_fit_hist_sm + k_fit_hnewton, whose 16-bit LDS bins shared by several samples take the 6 x 10^5 LDS atomics of a sample much better than 32-bit bins with every
// lane of a wave on the same few addresses; a workgroup that owns a CU's LDS also keeps the emission launches of the other lanes off that CU: the headline went from
// 3.9 to 4.07 ms per step.  What wins for a 10 000-cell column does not for a 200 000-cell one.)

}  // namespace
