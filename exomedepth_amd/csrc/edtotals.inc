// The core of the maps indexed by a cell's total n = test + ref (DESIGN.md 4.22): the detection-power map (edpower.inc), the quantile map
// (edquant.inc) and the draws from the fitted model (edsim.inc).  Under a sample's fitted beta-binomial a value depends on the exon through
// n alone, so all three walk a sample once per OCCUPIED total.  Here is what they share:
//   the occupancy passes (k_pw_scan .. k_pw_slots, pw_occupy): per sample the table of its occupied totals, the job list of the walk
//     (longest first) and per (sample, exon) the table slot of the exon's total;
//   the CDF walk (bb_open, bb_step) of the quantile map and the draws: one piece of source, so that both form C(x) from the same
//     operations and -- with -ffp-contract=off -- the same bits;
//   a resident map (TotalsMap: the occupancy and `channels` values per table entry) with its look-ups: the exon map, a sample's table,
//     the counters, and what the map and region entries check and stage alike.
// k_pw_walk (two hypotheses at once, moments in the log domain) is another walk and stays in edpower.inc.

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

// ---- the CDF walk --------------------------------------------------------------------------------------------------------------
// One wavefront walks pm[x], the mass of BetaBinomial(n, a, b) at x = 0 .. n (n > 0), and C(x) = pm[0] + .. + pm[x], in tiles of 64 lanes
// x 4 values.  With L(x) = log pm[x],
//   L(x + 1) - L(x) = log[(n - x)(a + x) / ((x + 1)(b + n - x - 1))]        L(0) = sum_{k < n} log[(b + k) / (a + b + k)]
// Step ratios multiplied four at a time, one logarithm per product, a wave scan of the logarithms on a log-domain carry (P(0) may
// underflow), exp once per lane, the four masses by products; a second wave scan of the lanes' mass sums on a running carry gives C.
// Sums in one fixed order: the bits of C depend on (n, a, b) alone.
struct BbWalk {
  int64_t n;
  double size, a, b;
  double carry_l, carry_c;      // L and C before the next tile's first value
};
// what one tile leaves in a lane: its values xs .. xs + 3
struct BbTile {
  int64_t xs;
  double m[edpower::kWalkPer], part[edpower::kWalkPer];      // the lane's masses and their running sums
  double excl, incl;                                          // C before the lane's first value, C at its last
  bool holds;                                                 // (a lane behind n holds no value to cross at)
};

__device__ __forceinline__ BbWalk bb_open(int64_t n, double a, double b, int lane)
{
  constexpr int P = edpower::kWalkPer;
  const double th = a + b;
  double sl = 0.0;
  for (int64_t k0 = (int64_t)lane * P; k0 < n; k0 += 64 * P) {
    double ql = 1.0;
#pragma unroll
    for (int j = 0; j < P; ++j)
      if (k0 + j < n) {
        const double kd = (double)(k0 + j);
        ql *= (b + kd) * edfit::frcp(th + kd);
      }
    sl += edfit::flog(ql);
  }
  return BbWalk{n, (double)n, a, b, pw_wave_sum(sl), 0.0};
}

// tile `tile` of the walk (the tiles are taken in order, each once); both carries move on to the next
__device__ __forceinline__ BbTile bb_step(BbWalk& w, int64_t tile, int lane)
{
  constexpr int P = edpower::kWalkPer;
  const int64_t n = w.n;
  const double size = w.size, a = w.a, b = w.b;
  BbTile t;
  const int64_t xs = t.xs = tile * edpower::kWalkTile + (int64_t)lane * P;
  double ql[P + 1];       // products of the step ratios before value j of the lane
  ql[0] = 1.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    double r = 1.0;
    if (xs + j < n) {
      const double xd = (double)(xs + j);
      const double rest = size - xd - 1.0;
      r = ((size - xd) * (a + xd)) * edfit::frcp((xd + 1.0) * (b + rest));
    }
    ql[j + 1] = ql[j] * r;
  }
  const double il = pw_wave_scan(edfit::flog(ql[P]), lane);
  const double el = __shfl_up(il, 1, 64);                         // the lanes before this one
  const double pr0 = ed_pexp(lane ? w.carry_l + el : w.carry_l);
#pragma unroll
  for (int j = 0; j < P; ++j) {
    t.m[j] = xs + j <= n ? pr0 * ql[j] : 0.0;
    t.part[j] = j ? t.part[j - 1] + t.m[j] : t.m[j];
  }
  const double is = pw_wave_scan(t.part[P - 1], lane);
  const double es = __shfl_up(is, 1, 64);
  t.excl = lane ? w.carry_c + es : w.carry_c;
  t.incl = t.excl + t.part[P - 1];
  t.holds = xs <= n;
  w.carry_l += __shfl(il, 63, 64);
  w.carry_c += __shfl(is, 63, 64);
  return t;
}

// ---- a resident map's exons ----------------------------------------------------------------------------------------------------
// the map of s1 - s0 samples, out [channels][s1 - s0][E]
__global__ void __launch_bounds__(256)
k_tm_exons(const int32_t* __restrict__ slot, const int64_t* __restrict__ tab_off, const double* __restrict__ val, int64_t J, int channels,
           int64_t E, int64_t s0, int64_t s1, double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ns = s1 - s0;
  if (i >= ns * E) return;
  const int64_t s = s0 + i / E;
  const int32_t sl = slot[s * E + i % E];
  const int64_t at = tab_off[s] + sl;
  for (int c = 0; c < channels; ++c) out[c * ns * E + i] = sl < 0 ? ed_pm_nan() : val[c * J + at];
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// What the occupancy passes leave behind for a map's look-ups: per sample the table of its occupied totals and per (sample, exon) the
// table slot of the exon's total.
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
// a resident map: the occupancy and `channels` values per table entry (ed_power, ed_quant)
struct TotalsMap : PwOccupancy {
  const ed_plan* plan = nullptr;
  int channels = 0;
  int64_t n_bad = 0;                 // samples outside the model
  DevBuf<double> d_val;              // [channels][J]
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

// the samples' shapes, qbetabinom's operations in its order (R/tools.R:22-23); returns the samples outside the model
int64_t sim_shapes(const double* phi, const double* expected, int64_t S, std::vector<double>& ab, std::vector<int32_t>& bad)
{
  ab.assign((size_t)S * 2, 0.0);
  bad.assign((size_t)S, 0);
  int64_t n_bad = 0;
  for (int64_t s = 0; s < S; ++s) {
    const double a = expected[s] * (1. - phi[s]) / phi[s], b = (1. - expected[s]) * (1. - phi[s]) / phi[s];
    ab[(size_t)s] = a; ab[(size_t)(S + s)] = b;
    bad[(size_t)s] = (a > 0.0 && b > 0.0 && a < HUGE_VAL && b < HUGE_VAL) ? 0 : 1;
    n_bad += bad[(size_t)s];
  }
  return n_bad;
}

// ---- what the entries of a resident map share; `entry` names the caller in the messages ----------------------------------------
// A map entry's arguments, the entry's own checks (`own`, after the shared ones and before a device is asked for), the device, and the
// counts staged: test / ref point at DEVICE arrays afterwards.
template <class Map, class Own>
int tm_map_begin(const char* entry, Map** out, const ed_plan* p, const int32_t*& test, const int32_t*& ref, int counts_on_device, int layout,
                 int64_t n_samples, const double* phi, const double* expected, Own own, DevBuf<int32_t>& up_test, DevBuf<int32_t>& up_ref,
                 hipStream_t st)
{
  if (!out) return ed_fail(ED_ERR_INVALID, "%s: NULL output", entry);
  *out = nullptr;
  if (!p) return ed_fail(ED_ERR_INVALID, "%s: NULL plan", entry);
  if (int rc = check_counts_args(entry, layout, n_samples)) return rc;
  if (!phi || !expected || (p->E > 0 && (!test || !ref))) return ed_fail(ED_ERR_INVALID, "%s: NULL array", entry);
  if (int rc = own()) return rc;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  return pw_stage_counts(entry, test, ref, counts_on_device, n_samples * p->E, up_test, up_ref, st);
}

int tm_regions_nomem(const char* entry, int64_t R, int64_t S)
{
  return ed_fail(ED_ERR_NOMEM, "%s: cannot allocate %lld rows x %lld samples", entry, (long long)R, (long long)S);
}

// A regions entry up to its own buffers: the arguments (have_out: none of the entry's outputs is NULL), every row, the device, the
// launch limit, and the rows on the device (the stream has been waited for).  With n_rows == 0 nothing is left to do.
int tm_regions_begin(const char* entry, const TotalsMap* m, const ed_call* rows, int64_t n_rows, bool have_out, DevBuf<ed_call>& d_rows,
                     hipStream_t st)
{
  if (!m) return ed_fail(ED_ERR_INVALID, "%s: NULL map", entry);
  if (n_rows < 0 || n_rows > (1 << 24)) return ed_fail(ED_ERR_INVALID, "%s: n_rows is outside 0 .. 16777216", entry);
  if (n_rows > 0 && (!rows || !have_out)) return ed_fail(ED_ERR_INVALID, "%s: NULL array", entry);
  if (int rc = check_region_rows(entry, m->plan, rows, n_rows)) return rc;
  if (n_rows == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(m->plan->device));
  const int64_t R = n_rows, S = m->S;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  if (R * sgroups > 0x7fffffffLL) return ed_fail(ED_ERR_INVALID, "%s: %lld rows x %lld samples are too many for one call", entry, (long long)R, (long long)S);
  if (d_rows.alloc((size_t)R * sizeof(ed_call)) != hipSuccess) return tm_regions_nomem(entry, R, S);
  HIP_TRY(hipMemcpyAsync(d_rows.get(), rows, (size_t)R * sizeof(ed_call), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ED_OK;
}

// The per-exon map to a HOST array [channels][S][E], made in groups of samples through a device buffer of at most 256 MiB
int tm_copy_exons(const char* entry, TotalsMap* m, double* out, void* stream)
{
  if (!m || !out) return ed_fail(ED_ERR_INVALID, "%s: NULL argument", entry);
  const int64_t S = m->S, E = m->E, CH = m->channels;
  if (E == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(m->plan->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t group = std::max<int64_t>(1, std::min<int64_t>(S, (int64_t)(256 << 20) / (E * CH * 8)));
  DevBuf<double> d_out;
  if (d_out.alloc((size_t)(group * E * CH) * 8) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "%s: cannot allocate %lld samples", entry, (long long)group);
  double ms = 0;
  for (int64_t s0 = 0; s0 < S; s0 += group) {
    const int64_t s1 = std::min(S, s0 + group), ns = s1 - s0;
    PwClock clock;
    hipLaunchKernelGGL(k_tm_exons, dim3((unsigned)((ns * E + 255) / 256)), dim3(256), 0, st, (const int32_t*)m->d_slot.get(),
                       (const int64_t*)m->d_tab_off.get(), (const double*)m->d_val.get(), m->J, m->channels, E, s0, s1, d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    ms += clock.lap();
    for (int64_t c = 0; c < CH; ++c)
      HIP_TRY(hipMemcpyAsync(out + (c * S + s0) * E, d_out.get() + c * ns * E, (size_t)ns * E * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  m->ms[3] = ms;
  return ED_OK;
}

// One sample's table: *n = its occupied totals; when cap >= *n, totals [*n] (ascending) and values [channels][cap] to HOST arrays
int tm_copy_table(const char* entry, const TotalsMap* m, int64_t sample, int32_t* totals, double* values, int64_t cap, int64_t* n)
{
  if (!m || !n || sample < 0 || sample >= m->S || cap < 0) return ed_fail(ED_ERR_INVALID, "%s: bad arguments", entry);
  const int64_t off = m->tab_off[(size_t)sample], k = m->tab_off[(size_t)sample + 1] - off;
  *n = k;
  if (cap < k || k == 0) return ED_OK;
  if (!totals || !values) return ed_fail(ED_ERR_INVALID, "%s: NULL array", entry);
  HIP_TRY(hipSetDevice(m->plan->device));
  HIP_TRY(hipMemcpy(totals, m->d_tab_n.get() + off, (size_t)k * 4, hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < m->channels; ++c)
    HIP_TRY(hipMemcpy(values + c * cap, m->d_val.get() + c * m->J + off, (size_t)k * 8, hipMemcpyDeviceToHost));
  return ED_OK;
}

// counts [8] = {samples, exons, jobs, most jobs of a sample, cells skipped, samples outside the model, largest valid total, words of a
// map row}; ms [4] (may be NULL) = {occupancy, walk, kernels of the last regions call, kernels of the last exon map}, host-timed between waits
void tm_stats(const TotalsMap& m, int64_t* counts, double* ms)
{
  counts[0] = m.S; counts[1] = m.E; counts[2] = m.J; counts[3] = m.max_jobs; counts[4] = m.n_skipped; counts[5] = m.n_bad;
  counts[6] = m.largest; counts[7] = m.words;
  if (ms) for (int i = 0; i < 4; ++i) ms[i] = m.ms[i];
}

// out [4] = {values of x a walk takes per tile, occupancy cap, largest total walked, exons a region step takes}
void tm_geometry(int32_t* out)
{
  out[0] = edpower::kWalkTile; out[1] = edpower::kOccCap; out[2] = edpower::kMaxTotal; out[3] = edpower::kRegionTile;
}
}  // namespace
