// The detection-power map: the expected Bayes factor of a heterozygous deletion / duplication of every exon, under the emission model
// CallCNVs decodes, and its sums over regions (DESIGN.md 4.22).
//
// Sample s has (phi, expected, mixture); sd = sqrt((phi * expected) * (1 - expected)); (a1_j, a2_j) = shape_params(state_props(expected,
// mixture)[j], sd) for j = deletion, normal, duplication -- the strict emissions' parameters.  For T in {deletion, duplication} and a total n:
//   X ~ BetaBinomial(n, a1_T, a2_T)      D_T(x) = log10(e) [e_T(x) - e_N(x)]      e_j(x) = lnbeta(a1_j + x, a2_j + n - x) - lnbeta(a1_j, a2_j)
//   mean_T = E[D_T(X)]  (a Kullback-Leibler divergence: >= 0)                       var_T = Var[D_T(X)]
// Both depend on the exon through n alone: a sample is walked once per OCCUPIED total (ed_power_plan.hpp), not once per exon.
//
// The walk (k_pw_walk) is k_rs_power_walk's (edrefset.inc) for both alternatives at once: with L_T(x) = log P_T(x),
//   L_T(x + 1) - L_T(x) = log[(n - x)(a1_T + x) / ((x + 1)(a2_T + n - x - 1))]
//   D_T(x + 1) - D_T(x) = log[(a1_T + x)(a2_N + n - x - 1) / ((a1_N + x)(a2_T + n - x - 1))]         (natural logarithms; scaled at the end)
//   L_T(0) = sum_{k < n} log[(a2_T + k) / (a1_T + a2_T + k)]      D_T(0) = sum_{k < n} log[(a2_T + k)(a1_N + a2_N + k) / ((a1_T + a2_T + k)(a2_N + k))]
// -- D_T(0) from its own products, not as a difference of two sums that cancel when the mixture is small.  Step ratios multiplied four
// at a time, one logarithm per product, a wave scan, the null's terms shared by the two alternatives; the variance in a second walk
// about the mean of the first.  Sums in a fixed order; no atomics on doubles anywhere in this file.
// The bits of a table value depend on (n, phi, expected, mixture) alone; those of a region value on its run and its sample alone.

namespace {

__device__ __forceinline__ int64_t pw_total(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t at)
{
  return (int64_t)test[at] + (int64_t)ref[at];
}

// ---- occupancy ----------------------------------------------------------------------------------------------------------------
// pass 1, over the cells in memory order (either layout): the largest valid total and the number of cells skipped
__global__ void __launch_bounds__(256)
k_pw_scan(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t n_cells, int32_t* __restrict__ gmax,
          unsigned long long* __restrict__ n_skipped)
{
  int32_t mx = 0;
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * 256) {
    const int64_t t = pw_total(test, ref, i);
    if (edpower::total_ok(t)) mx = max(mx, (int32_t)t); else ++bad;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mx = max(mx, __shfl_xor(mx, d, 64));
    bad += __shfl_xor(bad, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx > 0) atomicMax(gmax, mx);
    if (bad) atomicAdd(n_skipped, bad);
  }
}

// pass 2: the bit of every valid total into its sample's row.  The word is read first: after the first few cells of a sample nearly
// every bit is there already and no atomic is issued (a stale read costs a redundant atomic, nothing else).
__global__ void __launch_bounds__(256)
k_pw_mark(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t n_cells, int layout, int64_t E, int64_t S,
          int32_t words, unsigned int* __restrict__ bits)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * 256) {
    const int64_t t = pw_total(test, ref, i);
    if (!edpower::total_ok(t) || edpower::word_of((int32_t)t) >= words) continue;
    const int64_t s = layout ? i / E : i % S;
    const int32_t n = (int32_t)t;
    unsigned int* w = bits + s * words + edpower::word_of(n);          // word_of(n) < words: n <= the map's largest total (map_words)
    const unsigned int m = 1u << (n & 31);
    if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & m)) atomicOr(w, m);
  }
}

// pass 3, a workgroup per sample: prefix[s][w] = the set bits of the sample's words before w; count[s] = all of them
__global__ void __launch_bounds__(256)
k_pw_rank(const unsigned int* __restrict__ bits, int32_t words, int32_t* __restrict__ prefix, int32_t* __restrict__ count)
{
  __shared__ int32_t s_wave[4];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t base = 0;
  for (int32_t w0 = 0; w0 < words; w0 += 256) {
    const int32_t w = w0 + tid;
    const int32_t c = w < words ? __popc(bits[s * words + w]) : 0;
    int32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int32_t before = 0;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    const int32_t all = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (w < words) prefix[s * words + w] = base + before + inc - c;
    base += all;
    __syncthreads();
  }
  if (tid == 0) count[s] = base;
}

// pass 4, a thread per word: the sample's table of totals (ascending) and its jobs into the list (ed_power_plan.hpp: JobLayout)
__global__ void __launch_bounds__(256)
k_pw_jobs(const unsigned int* __restrict__ bits, const int32_t* __restrict__ prefix, const int32_t* __restrict__ count, int32_t words, int64_t S,
          const int64_t* __restrict__ tab_off, const int32_t* __restrict__ rank, const int64_t* __restrict__ off_k,
          int32_t* __restrict__ tab_n, int32_t* __restrict__ job_s, int32_t* __restrict__ job_n, int64_t* __restrict__ job_dst)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * words) return;
  const int64_t s = i / words;
  const int32_t w = (int32_t)(i % words);
  unsigned int word = bits[i];
  int32_t slot = prefix[i];
  const int32_t cnt = count[s];
  while (word) {
    const int b = __ffs((int)word) - 1;
    word &= word - 1;
    const int32_t n = w * 32 + b;
    const int64_t dst = tab_off[s] + slot;
    tab_n[dst] = n;
    const int64_t j = off_k[cnt - 1 - slot] + rank[s];
    job_s[j] = (int32_t)s; job_n[j] = n; job_dst[j] = dst;
    ++slot;
  }
}

// pass 5: slot[s][e] = the place of the exon's total in its sample's table, -1 for a skipped total.  A tile of 64 exons x 64 samples is
// read along the counts' own fast index and written along the exons.
__global__ void __launch_bounds__(256)
k_pw_slots(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int layout, int64_t E, int64_t S, int32_t words,
           const unsigned int* __restrict__ bits, const int32_t* __restrict__ prefix, int32_t* __restrict__ slot)
{
  constexpr int T = edpower::kSlotTile;
  __shared__ int32_t tile[T][T + 1];
  const int64_t e0 = (int64_t)blockIdx.x * T, s0 = (int64_t)blockIdx.y * T;
  const int fast = threadIdx.x & 63, slow = threadIdx.x >> 6;
  for (int r = 0; r < T / 4; ++r) {
    const int el = layout ? fast : r * 4 + slow, sl = layout ? r * 4 + slow : fast;
    const int64_t e = e0 + el, s = s0 + sl;
    if (e < E && s < S) {
      const int64_t t = pw_total(test, ref, layout ? s * E + e : e * S + s);
      int32_t v = -1;
      if (edpower::total_ok(t) && edpower::word_of((int32_t)t) < words) {
        const int32_t n = (int32_t)t;
        const int64_t at = s * words + edpower::word_of(n);
        v = prefix[at] + __popc(bits[at] & edpower::below_mask(n));
      }
      tile[el][sl] = v;
    }
  }
  __syncthreads();
  for (int r = 0; r < T / 4; ++r) {
    const int el = fast, sl = r * 4 + slow;
    const int64_t e = e0 + el, s = s0 + sl;
    if (e < E && s < S) slot[s * E + e] = tile[el][sl];
  }
}

// ---- the samples' parameters ---------------------------------------------------------------------------------------------------
// par [6][S]: a1, a2 of deletion, normal, duplication; bad[s] = 1 where they are not all positive and finite (phi too large for the model)
__global__ void k_pw_params(const double* __restrict__ phi, const double* __restrict__ expected, const double* __restrict__ mix_s, double mixture,
                            int64_t S, double* __restrict__ par, int32_t* __restrict__ bad)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double ex = expected[s];
  const double sd = __builtin_sqrt((phi[s] * ex) * (1. - ex));
  double ep[3];
  state_props(ex, mix_s ? mix_s[s] : mixture, ep);
  bool ok = true;
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    double a1, a2;
    shape_params(ep[st], sd, a1, a2);
    par[(2 * st) * S + s] = a1;
    par[(2 * st + 1) * S + s] = a2;
    ok = ok && a1 > 0.0 && a2 > 0.0 && a1 < HUGE_VAL && a2 < HUGE_VAL;
  }
  bad[s] = ok ? 0 : 1;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_pw_walk(const int32_t* __restrict__ job_s, const int32_t* __restrict__ job_n, const int64_t* __restrict__ job_dst, int64_t J,
          const double* __restrict__ par, const int32_t* __restrict__ bad, int64_t S, double* __restrict__ val)
{
  constexpr int P = edpower::kWalkPer;
  const int lane = threadIdx.x & 63;
  const int64_t jb = (int64_t)blockIdx.x * edpower::kWalkWaves + (threadIdx.x >> 6);
  if (jb >= J) return;
  const int64_t s = job_s[jb], dst = job_dst[jb];
  const int64_t n = job_n[jb];
  if (bad[s]) { if (lane < 4) val[lane * J + dst] = ed_pm_nan(); return; }
  if (n == 0) { if (lane < 4) val[lane * J + dst] = 0.0; return; }
  const double aN = par[2 * S + s], bN = par[3 * S + s];
  const double aT[2] = {par[s], par[4 * S + s]}, bT[2] = {par[S + s], par[5 * S + s]};
  const double thN = aN + bN, thT[2] = {aT[0] + bT[0], aT[1] + bT[1]};
  const double size = (double)n;
  // pass 1: L_T(0), D_T(0)
  double L0[2], D0[2];
  {
    double sl[2] = {0.0, 0.0}, sd[2] = {0.0, 0.0};
    for (int64_t k0 = (int64_t)lane * P; k0 < n; k0 += 64 * P) {
      double ql[2] = {1.0, 1.0}, qd[2] = {1.0, 1.0};
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (k0 + j < n) {
          const double kd = (double)(k0 + j);
          const double nb = bN + kd, nt = thN + kd;
#pragma unroll
          for (int T = 0; T < 2; ++T) {
            const double u = bT[T] + kd, v = thT[T] + kd;
            const double inv = edfit::frcp(v * nb);
            ql[T] *= (u * nb) * inv;
            qd[T] *= (u * nt) * inv;
          }
        }
      }
#pragma unroll
      for (int T = 0; T < 2; ++T) { sl[T] += edfit::flog(ql[T]); sd[T] += edfit::flog(qd[T]); }
    }
#pragma unroll
    for (int T = 0; T < 2; ++T) { L0[T] = pw_wave_sum(sl[T]); D0[T] = pw_wave_sum(sd[T]); }
  }
  // the walks: the mean, then the variance about it
  double mu[2] = {0.0, 0.0}, m2[2] = {0.0, 0.0};
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    double carry_l[2] = {L0[0], L0[1]}, carry_d[2] = {D0[0], D0[1]};
    double acc[2] = {0.0, 0.0};
    for (int64_t tile = 0; tile < edpower::n_walk_tiles(n); ++tile) {
      const int64_t xs = tile * edpower::kWalkTile + (int64_t)lane * P;
      double ql[2][P + 1], qd[2][P + 1];       // products of the step ratios before value j of the lane
      ql[0][0] = ql[1][0] = qd[0][0] = qd[1][0] = 1.0;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double rl[2] = {1.0, 1.0}, rd[2] = {1.0, 1.0};
        if (xs + j < n) {
          const double xd = (double)(xs + j);
          const double rest = size - xd - 1.0, w = aN + xd, t = bN + rest, x1 = xd + 1.0, up = size - xd;
#pragma unroll
          for (int T = 0; T < 2; ++T) {
            const double u = aT[T] + xd, v = bT[T] + rest;
            const double inv = edfit::frcp(x1 * v * w);
            rl[T] = (up * u) * w * inv;
            rd[T] = (u * t) * x1 * inv;
          }
        }
#pragma unroll
        for (int T = 0; T < 2; ++T) { ql[T][j + 1] = ql[T][j] * rl[T]; qd[T][j + 1] = qd[T][j] * rd[T]; }
      }
#pragma unroll
      for (int T = 0; T < 2; ++T) {
        const double ll = edfit::flog(ql[T][P]), ld = edfit::flog(qd[T][P]);
        const double il = pw_wave_scan(ll, lane), id = pw_wave_scan(ld, lane);
        const double el = __shfl_up(il, 1, 64), ed = __shfl_up(id, 1, 64);           // the lanes before this one
        const double base_l = lane ? carry_l[T] + el : carry_l[T], base_d = lane ? carry_d[T] + ed : carry_d[T];
        const double pr0 = ed_pexp(base_l);
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (xs + j <= n) {
            const double dj = (j == 0) ? base_d : base_d + edfit::flog(qd[T][j]);
            const double c = dj - mu[T];
            acc[T] = __builtin_fma(pr0 * ql[T][j], pass ? c * c : dj, acc[T]);
          }
        carry_l[T] += __shfl(il, 63, 64);
        carry_d[T] += __shfl(id, 63, 64);
      }
    }
#pragma unroll
    for (int T = 0; T < 2; ++T) {
      const double v = pw_wave_sum(acc[T]);
      if (pass == 0) mu[T] = v; else m2[T] = v;
    }
  }
  constexpr double M = 0.43429448190325182765;      // log10(e)
  if (lane == 0) {
    val[0 * J + dst] = M * mu[0];
    val[1 * J + dst] = (M * M) * m2[0];
    val[2 * J + dst] = M * mu[1];
    val[3 * J + dst] = (M * M) * m2[1];
  }
}

// ---- exons and regions ---------------------------------------------------------------------------------------------------------
// the map of s1 - s0 samples, out [4][s1 - s0][E]
__global__ void __launch_bounds__(256)
k_pw_exons(const int32_t* __restrict__ slot, const int64_t* __restrict__ tab_off, const double* __restrict__ val, int64_t J, int64_t E,
           int64_t s0, int64_t s1, double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ns = s1 - s0;
  if (i >= ns * E) return;
  const int64_t s = s0 + i / E;
  const int32_t sl = slot[s * E + i % E];
  const int64_t at = tab_off[s] + sl;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c * ns * E + i] = sl < 0 ? ed_pm_nan() : val[c * J + at];
}

// rows [R] of (chromosome, first, last); a wavefront per (row, sample): sums [4][R][S] and empty [R][S] in ed_power_plan.hpp's order
__global__ void __launch_bounds__(edpower::kRegionWaves * 64)
k_pw_regions(const ed_call* __restrict__ rows, int64_t R, const int32_t* __restrict__ slot, const int64_t* __restrict__ tab_off,
             const int32_t* __restrict__ tab_n, const double* __restrict__ val, int64_t J, int64_t E, int64_t S, double* __restrict__ sums,
             int32_t* __restrict__ empty)
{
  const int lane = threadIdx.x & 63;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  const int64_t r = blockIdx.x / sgroups;
  const int64_t s = (blockIdx.x % sgroups) * edpower::kRegionWaves + (threadIdx.x >> 6);
  if (r >= R || s >= S) return;
  const int64_t first = rows[r].start_exon, len = (int64_t)rows[r].end_exon - first + 1;
  const int64_t off = tab_off[s];
  const bool has0 = tab_off[s + 1] > off && tab_n[off] == 0;        // the table is ascending: a total of 0 is its slot 0
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t ne = 0;
  for (int64_t i = lane; i < len; i += edpower::kRegionTile) {
    const int32_t sl = slot[s * E + first + i];
    ne += (sl == 0 && has0) ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += sl < 0 ? ed_pm_nan() : val[c * J + off + sl];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += __shfl_xor(acc[c], d, 64);
    ne += __shfl_xor(ne, d, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) sums[(c * R + r) * S + s] = acc[c];
    empty[r * S + s] = ne;
  }
}

// the price of a row, a wavefront per row: log10(e) (sum of N->N over the run's gaps - (N->T + sum of T->T over the inner gaps + T->N))
__global__ void __launch_bounds__(256)
k_pw_price(const ed_call* __restrict__ rows, int64_t R, const double* __restrict__ lt4, double c0, double c1, double* __restrict__ price)
{
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int32_t c = rows[r].chrom;
  const edpower::PriceGaps g = edpower::price_gaps(rows[r].start_exon, rows[r].end_exon, c);
  double acc = 0.0;
  for (int64_t row = g.inner0 + lane; row < g.inner1; row += 64) acc += lt4[row * 8 + 2];      // T->T of the inner gaps
  acc = pw_wave_sum(acc);
  if (lane == 0) {
    const double call = (c1 + acc) + lt4[g.close * 8];                                  // ... + T->N of the gap behind the run
    price[r] = 0.43429448190325182765 * ((double)g.n_nn * c0 - call);
  }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// What the occupancy passes leave behind for a map's look-ups: per sample the table of its occupied totals and per (sample, exon) the
// table slot of the exon's total.  The quantile map (edquant.inc) is built on the same.
struct PwOccupancy {
  int64_t S = 0, E = 0, J = 0;
  int32_t words = 0, largest = 0, max_jobs = 0;
  int64_t n_skipped = 0;
  std::vector<int64_t> tab_off;      // [S + 1]
  DevBuf<int64_t> d_tab_off;         // [S + 1]
  DevBuf<int32_t> d_slot;            // [S][E]
  DevBuf<int32_t> d_tab_n;           // [J]
};
// the job list of a walk, longest first (ed_power_plan.hpp: JobLayout); the walk's own, gone with it
struct PwJobs {
  DevBuf<int32_t> d_s, d_n;          // [J] sample, total
  DevBuf<int64_t> d_dst;             // [J] place in the tables
};

struct ed_power : PwOccupancy {
  const ed_plan* plan = nullptr;
  int64_t n_bad = 0;
  DevBuf<double> d_val;              // [4][J]  mean_del, var_del, mean_dup, var_dup
  double ms[4] = {0, 0, 0, 0};       // occupancy, walk, the last regions call's kernels, the last exon map's kernels
};

namespace {
struct PwClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap()
  {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};
inline unsigned pw_grid(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 1 << 20)); }

// host counts go to the device (up_test / up_ref own the copies); test / ref point at the device arrays afterwards
int pw_stage_counts(const char* entry, const int32_t*& test, const int32_t*& ref, int counts_on_device, int64_t cells, DevBuf<int32_t>& up_test,
                    DevBuf<int32_t>& up_ref, hipStream_t st)
{
  if (counts_on_device || cells <= 0) return ED_OK;
  if (up_test.alloc((size_t)cells * 4) != hipSuccess || up_ref.alloc((size_t)cells * 4) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "%s: cannot allocate the counts", entry);
  HIP_TRY(hipMemcpyAsync(up_test.get(), test, (size_t)cells * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(up_ref.get(), ref, (size_t)cells * 4, hipMemcpyHostToDevice, st));
  test = up_test.get(); ref = up_ref.get();
  return ED_OK;
}

// The occupancy passes over DEVICE counts: o (S and E set by the caller) and the job list.  Complete when it returns (it waits for st).
int pw_occupy(const char* entry, PwOccupancy& o, PwJobs& jobs, const int32_t* test, const int32_t* ref, int layout, hipStream_t st)
{
  const int64_t S = o.S, E = o.E, cells = S * E;
  o.tab_off.assign((size_t)S + 1, 0);
  auto nomem = [&](const char* what) { return ed_fail(ED_ERR_NOMEM, "%s: cannot allocate %s", entry, what); };
  DevBuf<int64_t> d_word;       // [0] the largest valid total (int32), [1] the cells skipped
  if (d_word.alloc(16) != hipSuccess) return nomem("counters");
  HIP_TRY(hipMemsetAsync(d_word.get(), 0, 16, st));
  if (cells > 0) {
    hipLaunchKernelGGL(k_pw_scan, dim3(pw_grid(cells, 256 * 8)), dim3(256), 0, st, test, ref, cells, (int32_t*)d_word.get(),
                       (unsigned long long*)(d_word.get() + 1));
    HIP_TRY(hipGetLastError());
  }
  int64_t word[2] = {0, 0};
  if (int rc = ed_d2h(word, d_word.get(), 16, st)) return rc;
  o.largest = (int32_t)(word[0] & 0xffffffff);
  o.n_skipped = word[1];
  const int32_t words = o.words = edpower::map_words(o.largest);
  DevBuf<unsigned int> d_bits;
  DevBuf<int32_t> d_prefix, d_count;
  if (d_bits.alloc((size_t)S * words * 4) != hipSuccess || d_prefix.alloc((size_t)S * words * 4) != hipSuccess ||
      d_count.alloc((size_t)S * 4) != hipSuccess || o.d_slot.alloc((size_t)std::max<int64_t>(cells, 1) * 4) != hipSuccess ||
      o.d_tab_off.alloc((size_t)(S + 1) * 8) != hipSuccess)
    return nomem("the occupancy map");
  HIP_TRY(hipMemsetAsync(d_bits.get(), 0, (size_t)S * words * 4, st));
  if (cells > 0) {
    hipLaunchKernelGGL(k_pw_mark, dim3(pw_grid(cells, 256 * 8)), dim3(256), 0, st, test, ref, cells, layout, E, S, words, d_bits.get());
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pw_rank, dim3((unsigned)S), dim3(256), 0, st, (const unsigned int*)d_bits.get(), words, d_prefix.get(), d_count.get());
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> count((size_t)S);
  if (int rc = ed_d2h(count.data(), d_count.get(), (size_t)S * 4, st)) return rc;
  for (int64_t s = 0; s < S; ++s) o.tab_off[(size_t)s + 1] = o.tab_off[(size_t)s] + count[(size_t)s];
  const edpower::JobLayout lay = edpower::job_layout(count.data(), S);
  const int64_t J = o.J = lay.n_jobs;
  o.max_jobs = lay.max_jobs;
  if (J != o.tab_off[(size_t)S]) return ed_fail(ED_ERR_STATE, "%s: internal error, the job list does not cover the tables", entry);
  HIP_TRY(hipMemcpyAsync(o.d_tab_off.get(), o.tab_off.data(), (size_t)(S + 1) * 8, hipMemcpyHostToDevice, st));
  DevBuf<int32_t> d_rank;
  DevBuf<int64_t> d_off_k;
  const size_t Ja = (size_t)std::max<int64_t>(J, 1);
  if (d_rank.alloc((size_t)S * 4) != hipSuccess || d_off_k.alloc(lay.off_k.size() * 8) != hipSuccess || jobs.d_s.alloc(Ja * 4) != hipSuccess ||
      jobs.d_n.alloc(Ja * 4) != hipSuccess || jobs.d_dst.alloc(Ja * 8) != hipSuccess || o.d_tab_n.alloc(Ja * 4) != hipSuccess)
    return nomem("the job list");
  HIP_TRY(hipMemcpyAsync(d_rank.get(), lay.rank.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_off_k.get(), lay.off_k.data(), lay.off_k.size() * 8, hipMemcpyHostToDevice, st));
  if (J > 0) {
    hipLaunchKernelGGL(k_pw_jobs, dim3((unsigned)((S * words + 255) / 256)), dim3(256), 0, st, (const unsigned int*)d_bits.get(),
                       (const int32_t*)d_prefix.get(), (const int32_t*)d_count.get(), words, S, (const int64_t*)o.d_tab_off.get(),
                       (const int32_t*)d_rank.get(), (const int64_t*)d_off_k.get(), o.d_tab_n.get(), jobs.d_s.get(), jobs.d_n.get(), jobs.d_dst.get());
    HIP_TRY(hipGetLastError());
  }
  if (cells > 0) {
    constexpr int T = edpower::kSlotTile;
    if ((S + T - 1) / T > 65535) return ed_fail(ED_ERR_INVALID, "%s: too many samples for one map", entry);
    hipLaunchKernelGGL(k_pw_slots, dim3((unsigned)((E + T - 1) / T), (unsigned)((S + T - 1) / T)), dim3(256), 0, st, test, ref, layout, E, S, words,
                       (const unsigned int*)d_bits.get(), (const int32_t*)d_prefix.get(), o.d_slot.get());
    HIP_TRY(hipGetLastError());
  }
  // (the passes read d_bits, d_prefix, d_rank and d_off_k, which go when this returns)
  HIP_TRY(hipStreamSynchronize(st));
  return ED_OK;
}
}  // namespace

// The map of n_samples samples of the plan's exons.  test / ref: int32 counts, [E][S] (layout 0) or [S][E] (layout 1), on the device
// (counts_on_device != 0) or on the host; phi, expected, mixture_s: HOST arrays [S]; mixture_s NULL: `mixture` for every sample.
// Complete when it returns (it waits for `stream`); the counts are not needed afterwards.  The plan must outlive the map.
ED_EXPORT int ed_plan_power_map(ed_power** out, const ed_plan* p, const int32_t* test, const int32_t* ref, int counts_on_device, int layout,
                                int64_t n_samples, const double* phi, const double* expected, const double* mixture_s, double mixture,
                                void* stream)
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_plan_power_map: NULL output");
  *out = nullptr;
  if (!p) return ed_fail(ED_ERR_INVALID, "ed_plan_power_map: NULL plan");
  if (int rc = check_counts_args("ed_plan_power_map", layout, n_samples)) return rc;
  if (!phi || !expected || (p->E > 0 && (!test || !ref))) return ed_fail(ED_ERR_INVALID, "ed_plan_power_map: NULL array");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = n_samples, E = p->E;
  std::unique_ptr<ed_power> h(new ed_power);
  h->plan = p; h->S = S; h->E = E;
  auto nomem = [&](const char* what) { return ed_fail(ED_ERR_NOMEM, "ed_plan_power_map: cannot allocate %s", what); };

  DevBuf<int32_t> up_test, up_ref;
  if (int rc = pw_stage_counts("ed_plan_power_map", test, ref, counts_on_device, S * E, up_test, up_ref, st)) return rc;
  // the samples' parameters
  DevBuf<double> d_in, d_par;
  DevBuf<int32_t> d_bad;
  if (d_in.alloc((size_t)S * 3 * 8) != hipSuccess || d_par.alloc((size_t)S * 6 * 8) != hipSuccess || d_bad.alloc((size_t)S * 4) != hipSuccess)
    return nomem("the samples' parameters");
  HIP_TRY(hipMemcpyAsync(d_in.get(), phi, (size_t)S * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in.get() + S, expected, (size_t)S * 8, hipMemcpyHostToDevice, st));
  if (mixture_s) HIP_TRY(hipMemcpyAsync(d_in.get() + 2 * S, mixture_s, (size_t)S * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pw_params, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (const double*)d_in.get(), (const double*)(d_in.get() + S),
                     mixture_s ? (const double*)(d_in.get() + 2 * S) : (const double*)nullptr, mixture, S, d_par.get(), d_bad.get());
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> bad((size_t)S);
  if (int rc = ed_d2h(bad.data(), d_bad.get(), (size_t)S * 4, st)) return rc;
  for (int32_t b : bad) h->n_bad += b;

  PwClock clock;
  PwJobs jobs;
  if (int rc = pw_occupy("ed_plan_power_map", *h, jobs, test, ref, layout, st)) return rc;
  const int64_t J = h->J;
  if (h->d_val.alloc((size_t)std::max<int64_t>(J, 1) * 4 * 8) != hipSuccess) return nomem("the tables");
  h->ms[0] = clock.lap();
  // the walk
  if (J > 0) {
    hipLaunchKernelGGL(k_pw_walk, dim3((unsigned)((J + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, st,
                       (const int32_t*)jobs.d_s.get(), (const int32_t*)jobs.d_n.get(), (const int64_t*)jobs.d_dst.get(), J, (const double*)d_par.get(),
                       (const int32_t*)d_bad.get(), S, h->d_val.get());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  h->ms[1] = clock.lap();
  *out = h.release();
  return ED_OK;
}
ED_CATCH("ed_plan_power_map")

ED_EXPORT void ed_power_free(ed_power* pm) { delete pm; }

// Region rows (chrom, start_exon, end_exon of a call row; the other fields are not read) against every sample, to HOST arrays:
// sums [4][n_rows][S] (mean_del, var_del, mean_dup, var_dup), n_empty [n_rows][S], price [n_rows], n_exons [n_rows].  Every row is
// checked before anything is enqueued.
ED_EXPORT int ed_power_regions(ed_power* pm, const ed_call* rows, int64_t n_rows, double* sums, int32_t* n_empty, double* price,
                               int32_t* n_exons, void* stream)
try {
  if (!pm) return ed_fail(ED_ERR_INVALID, "ed_power_regions: NULL map");
  if (n_rows < 0 || n_rows > (1 << 24)) return ed_fail(ED_ERR_INVALID, "ed_power_regions: n_rows is outside 0 .. 16777216");
  if (n_rows > 0 && (!rows || !sums || !n_empty || !price || !n_exons)) return ed_fail(ED_ERR_INVALID, "ed_power_regions: NULL array");
  const ed_plan* p = pm->plan;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int f = edrows::row_fault(rows[r].chrom, rows[r].start_exon, rows[r].end_exon, p->C, p->chrom_off.data());
    if (f == 1) return ed_fail(ED_ERR_INVALID, "ed_power_regions: row %lld has first > last", (long long)r);
    if (f == 2) return ed_fail(ED_ERR_INVALID, "ed_power_regions: row %lld names a chromosome outside the plan", (long long)r);
    if (f == 3)
      return ed_fail(ED_ERR_INVALID, "ed_power_regions: row %lld does not lie inside its chromosome (it leaves the plan or crosses a boundary)",
                     (long long)r);
  }
  if (n_rows == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = n_rows, S = pm->S;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  if (R * sgroups > 0x7fffffffLL) return ed_fail(ED_ERR_INVALID, "ed_power_regions: %lld rows x %lld samples are too many for one call", (long long)R, (long long)S);
  DevBuf<ed_call> d_rows;
  DevBuf<double> d_sums, d_price;
  DevBuf<int32_t> d_empty;
  if (d_rows.alloc((size_t)R * sizeof(ed_call)) != hipSuccess || d_sums.alloc((size_t)R * S * 4 * 8) != hipSuccess ||
      d_price.alloc((size_t)R * 8) != hipSuccess || d_empty.alloc((size_t)R * S * 4) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_power_regions: cannot allocate %lld rows x %lld samples", (long long)R, (long long)S);
  HIP_TRY(hipMemcpyAsync(d_rows.get(), rows, (size_t)R * sizeof(ed_call), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  PwClock clock;
  hipLaunchKernelGGL(k_pw_regions, dim3((unsigned)(R * sgroups)), dim3(edpower::kRegionWaves * 64), 0, st, (const ed_call*)d_rows.get(), R,
                     (const int32_t*)pm->d_slot.get(), (const int64_t*)pm->d_tab_off.get(), (const int32_t*)pm->d_tab_n.get(),
                     (const double*)pm->d_val.get(), pm->J, pm->E, S, d_sums.get(), d_empty.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_pw_price, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, (const ed_call*)d_rows.get(), R, (const double*)p->d_lt3.get(),
                     p->c0, p->c1, d_price.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  pm->ms[2] = clock.lap();
  HIP_TRY(hipMemcpyAsync(sums, d_sums.get(), (size_t)R * S * 4 * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(n_empty, d_empty.get(), (size_t)R * S * 4, hipMemcpyDeviceToHost, st));
  if (int rc = ed_d2h(price, d_price.get(), (size_t)R * 8, st)) return rc;
  for (int64_t r = 0; r < R; ++r) n_exons[r] = rows[r].end_exon - rows[r].start_exon + 1;
  return ED_OK;
}
ED_CATCH("ed_power_regions")

// The per-exon map to a HOST array [4][S][E] (mean_del, var_del, mean_dup, var_dup); NaN where the exon's total was skipped or the
// sample's parameters are outside the model.  Made in groups of samples through a bounded device buffer.
ED_EXPORT int ed_power_copy_exons(ed_power* pm, double* out, void* stream)
try {
  if (!pm || !out) return ed_fail(ED_ERR_INVALID, "ed_power_copy_exons: NULL argument");
  const int64_t S = pm->S, E = pm->E;
  if (E == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(pm->plan->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t group = std::max<int64_t>(1, std::min<int64_t>(S, (int64_t)(256 << 20) / (E * 32)));
  DevBuf<double> d_out;
  if (d_out.alloc((size_t)group * E * 32) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "ed_power_copy_exons: cannot allocate %lld samples", (long long)group);
  double ms = 0;
  for (int64_t s0 = 0; s0 < S; s0 += group) {
    const int64_t s1 = std::min(S, s0 + group), ns = s1 - s0;
    PwClock clock;
    hipLaunchKernelGGL(k_pw_exons, dim3((unsigned)((ns * E + 255) / 256)), dim3(256), 0, st, (const int32_t*)pm->d_slot.get(),
                       (const int64_t*)pm->d_tab_off.get(), (const double*)pm->d_val.get(), pm->J, E, s0, s1, d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    ms += clock.lap();
    for (int c = 0; c < 4; ++c)
      HIP_TRY(hipMemcpyAsync(out + ((int64_t)c * S + s0) * E, d_out.get() + (int64_t)c * ns * E, (size_t)ns * E * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  pm->ms[3] = ms;
  return ED_OK;
}
ED_CATCH("ed_power_copy_exons")

// One sample's table: *n = its occupied totals; when cap >= *n, totals [*n] (ascending) and values [4][cap] to HOST arrays
ED_EXPORT int ed_power_copy_table(const ed_power* pm, int64_t sample, int32_t* totals, double* values, int64_t cap, int64_t* n)
try {
  if (!pm || !n || sample < 0 || sample >= pm->S || cap < 0) return ed_fail(ED_ERR_INVALID, "ed_power_copy_table: bad arguments");
  const int64_t off = pm->tab_off[(size_t)sample], k = pm->tab_off[(size_t)sample + 1] - off;
  *n = k;
  if (cap < k || k == 0) return ED_OK;
  if (!totals || !values) return ed_fail(ED_ERR_INVALID, "ed_power_copy_table: NULL array");
  HIP_TRY(hipSetDevice(pm->plan->device));
  HIP_TRY(hipMemcpy(totals, pm->d_tab_n.get() + off, (size_t)k * 4, hipMemcpyDeviceToHost));
  for (int c = 0; c < 4; ++c) HIP_TRY(hipMemcpy(values + (int64_t)c * cap, pm->d_val.get() + (int64_t)c * pm->J + off, (size_t)k * 8, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_power_copy_table")

// counts = {samples, exons, jobs, most jobs of a sample, cells skipped, samples outside the model, largest valid total, words of a map row};
// ms = {occupancy, walk, kernels of the last ed_power_regions, kernels of the last ed_power_copy_exons}, host-timed between waits
ED_EXPORT int ed_power_stats(const ed_power* pm, int64_t counts[8], double ms[4])
try {
  if (!pm || !counts) return ed_fail(ED_ERR_INVALID, "ed_power_stats: NULL argument");
  counts[0] = pm->S; counts[1] = pm->E; counts[2] = pm->J; counts[3] = pm->max_jobs; counts[4] = pm->n_skipped; counts[5] = pm->n_bad;
  counts[6] = pm->largest; counts[7] = pm->words;
  if (ms) for (int i = 0; i < 4; ++i) ms[i] = pm->ms[i];
  return ED_OK;
}
ED_CATCH("ed_power_stats")

// out = {values of x a walk takes per tile, occupancy cap, largest total walked, exons a region step takes}
ED_EXPORT int ed_power_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_power_geometry: NULL output");
  out[0] = edpower::kWalkTile; out[1] = edpower::kOccCap; out[2] = edpower::kMaxTotal; out[3] = edpower::kRegionTile;
  return ED_OK;
}
ED_CATCH("ed_power_geometry")
