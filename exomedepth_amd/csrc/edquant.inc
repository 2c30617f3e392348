// The quantile map: qbetabinom / qbetabinom.ab of the reference (R/tools.R:21-53) for every exon of every sample under the sample's fitted
// normal state, the band its plot draws (R/plot_CNVs_method.R:54-63), and per region how the observed counts fall between the quantiles
// (DESIGN.md 4.24).
//
// For a size n, shapes (a, b) and a probability p: pm[x] = the beta-binomial mass at x = 0 .. n, C(x) = pm[0] + .. + pm[x], cut = the
// smallest x with C(x) > p,
//   q = cut + (p - C(cut - 1)) / pm[cut]        (C(-1) = 0, so q = p / pm[0] for cut = 0)          below = C(cut - 1)
// -- `below` and `above` of qbetabinom.ab with R's 1-based indices written out.  No x with C(x) > p (p >= 1, or within rounding of 1):
// NaN, R's NA, in both.  n = 0: q = p.  Sample s has a = expected (1 - phi) / phi, b = (1 - expected)(1 - phi) / phi in qbetabinom's own
// operation order (NOT the emissions' shape_params: the same numbers, other roundings), formed on the host.
// Both depend on the exon through n alone: a sample is walked once per OCCUPIED total.  Occupancy, job list, slots, the resident map and
// its look-ups: edtotals.inc's.
//
// The walk (bq_walk) takes pm and C from the CDF walk of edtotals.inc (bb_open, bb_step: k_pw_walk's scheme for one distribution), tile
// by tile: lane l's C before its first value is `excl`, after its j-th the lane's own partial sum part[j] on top of that.  For each
// probability in turn a ballot finds the first lane whose last C exceeds it; that lane finds the value among its four.  The walk ends
// with the tile in which the last probability was crossed.  Sums in one fixed order, no atomics on doubles: the bits of a value depend
// on (n, a, b, p) alone -- not on the other probabilities of the request, which only decide where the walk ends.

namespace {

// One wavefront: the quantiles of BetaBinomial(n, a, b) at probs[0 .. K), ascending and the same in every lane; a probability >= 1 or NaN
// is never crossed.  The crossing lane writes q_out[k * stride] and below_out[k * stride].  Returns the tiles walked.
__device__ __forceinline__ int32_t bq_walk(int64_t n, double a, double b, const double* __restrict__ probs, int K, int lane,
                                           double* __restrict__ q_out, double* __restrict__ below_out, int64_t stride)
{
  constexpr int P = edpower::kWalkPer;
  if (n == 0) {
    if (lane < K) {
      const double p = probs[lane];
      const bool in = p < 1.0;
      q_out[lane * stride] = in ? p : ed_pm_nan();
      below_out[lane * stride] = in ? 0.0 : ed_pm_nan();
    }
    return 0;
  }
  BbWalk w = bb_open(n, a, b, lane);
  int done = 0;
  int32_t tiles = 0;
  const int64_t nt = edpower::n_walk_tiles(n);
  for (int64_t tile = 0; tile < nt && done < K; ++tile) {
    ++tiles;
    const BbTile c = bb_step(w, tile, lane);
    while (done < K) {
      const double p = probs[done];
      const unsigned long long hit = __ballot(p < 1.0 && c.holds && c.incl > p);
      if (!hit) break;
      if (lane == __ffsll((long long)hit) - 1) {
        // the first of the four whose C exceeds p: the last does
        int j = P - 1;
        double below = c.excl + c.part[P - 2], mass = c.m[P - 1];
#pragma unroll
        for (int t = P - 2; t >= 0; --t)
          if (c.excl + c.part[t] > p) { j = t; below = t ? c.excl + c.part[t - 1] : c.excl; mass = c.m[t]; }
        // (a `below` above p, or a mass of 0, can only come from the last bit of the two scans: the value itself then)
        const double frac = mass > 0.0 ? (p - below) * edfit::frcp(mass) : 0.0;
        q_out[done * stride] = (double)(c.xs + j) + frac;
        below_out[done * stride] = below;
      }
      ++done;
    }
  }
  if (lane == 0)
    for (int k = done; k < K; ++k) { q_out[k * stride] = ed_pm_nan(); below_out[k * stride] = ed_pm_nan(); }
  return tiles;
}

// val [2][K][J]: q, below; ab [2][S]; tiles [J]
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_bq_walk(const int32_t* __restrict__ job_s, const int32_t* __restrict__ job_n, const int64_t* __restrict__ job_dst, int64_t J,
          const double* __restrict__ ab, const int32_t* __restrict__ bad, int64_t S, const double* __restrict__ probs, int K,
          double* __restrict__ val, int32_t* __restrict__ tiles)
{
  const int lane = threadIdx.x & 63;
  const int64_t jb = (int64_t)blockIdx.x * edpower::kWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (jb >= J) return;
  const int64_t s = job_s[jb], dst = job_dst[jb];
  const int64_t n = job_n[jb];
  double* q_out = val + dst;
  double* below_out = val + (int64_t)K * J + dst;
  if (bad[s]) {
    if (lane < K) { q_out[lane * J] = ed_pm_nan(); below_out[lane * J] = ed_pm_nan(); }
    if (lane == 0) tiles[jb] = 0;
    return;
  }
  const int32_t t = bq_walk(n, ab[s], ab[S + s], probs, K, lane, q_out, below_out, J);
  if (lane == 0) tiles[jb] = t;
}

// the element-wise form: a wavefront per (p, size, a, b); NaN where the shapes are not positive and finite or the size is not a whole
// number in 0 .. the largest total walked
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_bq_points(const double* __restrict__ p, const double* __restrict__ size, const double* __restrict__ a, const double* __restrict__ b, int64_t N,
            double* __restrict__ q, double* __restrict__ below)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * edpower::kWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= N) return;
  const double sz = size[i], sa = a[i], sb = b[i];
  const bool ok = sa > 0.0 && sb > 0.0 && sa < HUGE_VAL && sb < HUGE_VAL && sz >= 0.0 && sz <= (double)edpower::kMaxTotal && (double)(int64_t)sz == sz;
  if (!ok) {
    if (lane == 0) { q[i] = ed_pm_nan(); below[i] = ed_pm_nan(); }
    return;
  }
  bq_walk((int64_t)sz, sa, sb, p + i, 1, lane, q + i, below + i, 1);
}

// the tiles walked and the tiles of full walks, out [2]
__global__ void __launch_bounds__(256)
k_bq_tally(const int32_t* __restrict__ job_n, const int32_t* __restrict__ tiles, int64_t J, unsigned long long* __restrict__ out)
{
  unsigned long long walked = 0, full = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < J; i += (int64_t)gridDim.x * 256) {
    walked += (unsigned long long)tiles[i];
    full += (unsigned long long)edpower::n_walk_tiles(job_n[i]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    walked += __shfl_xor(walked, d, 64);
    full += __shfl_xor(full, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, walked);
    atomicAdd(out + 1, full);
  }
}

// obs [S][E] = the test counts, read along the counts' own fast index and written along the exons (k_pw_slots' tiles)
__global__ void __launch_bounds__(256)
k_bq_obs(const int32_t* __restrict__ test, int layout, int64_t E, int64_t S, int32_t* __restrict__ obs)
{
  constexpr int T = edpower::kSlotTile;
  __shared__ int32_t tile[T][T + 1];
  const int64_t e0 = (int64_t)blockIdx.x * T, s0 = (int64_t)blockIdx.y * T;
  const int fast = threadIdx.x & 63, slow = threadIdx.x >> 6;
  for (int r = 0; r < T / 4; ++r) {
    const int el = layout ? fast : r * 4 + slow, sl = layout ? r * 4 + slow : fast;
    const int64_t e = e0 + el, s = s0 + sl;
    if (e < E && s < S) tile[el][sl] = test[layout ? s * E + e : e * S + s];
  }
  __syncthreads();
  for (int r = 0; r < T / 4; ++r) {
    const int el = fast, sl = r * 4 + slow;
    const int64_t e = e0 + el, s = s0 + sl;
    if (e < E && s < S) obs[s * E + e] = tile[el][sl];
  }
}

// rows [R] of (chromosome, first, last); a wavefront per (row, sample).  An exon whose total was skipped, or of a sample outside the
// model, is counted in empty and nowhere else.  The others: bin = the number of k with obs >= cut_of(q_k) (ed_quant_plan.hpp);
// observed [R][S][K + 1] counts them, expected [R][S][K + 1] adds below_{b+1} - below_b (below_0 = 0, below_{K+1} = 1) in
// ed_power_plan.hpp's region order.
__global__ void __launch_bounds__(edpower::kRegionWaves * 64)
k_bq_regions(const ed_call* __restrict__ rows, int64_t R, const int32_t* __restrict__ slot, const int32_t* __restrict__ obs,
             const int64_t* __restrict__ tab_off, const double* __restrict__ val, const int32_t* __restrict__ bad, int64_t J, int K, int64_t E,
             int64_t S, int32_t* __restrict__ observed, double* __restrict__ expected, int32_t* __restrict__ empty)
{
  constexpr int KB = edquant::kMaxProbs + 1;
  const int lane = threadIdx.x & 63;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  const int64_t r = blockIdx.x / sgroups;
  const int64_t s = (blockIdx.x % sgroups) * edpower::kRegionWaves + (threadIdx.x >> 6);
  if (r >= R || s >= S) return;
  const int64_t first = rows[r].start_exon, len = (int64_t)rows[r].end_exon - first + 1;
  const int64_t off = tab_off[s];
  const bool out_of_model = bad[s] != 0;
  double acc[KB];
  int32_t cnt[KB];
#pragma unroll
  for (int b = 0; b < KB; ++b) { acc[b] = 0.0; cnt[b] = 0; }
  int32_t ne = 0;
  for (int64_t i = lane; i < len; i += edpower::kRegionTile) {
    const int32_t sl = slot[s * E + first + i];
    if (sl < 0 || out_of_model) { ++ne; continue; }
    const int64_t ob = obs[s * E + first + i];
    const int64_t at = off + sl;
    double prev = 0.0;
    int bin = 0;
#pragma unroll
    for (int k = 0; k < edquant::kMaxProbs; ++k)
      if (k < K) {
        const double q = val[(int64_t)k * J + at], bl = val[(int64_t)(K + k) * J + at];
        bin += ob >= edquant::cut_of(q) ? 1 : 0;
        acc[k] += bl - prev;
        prev = bl;
      }
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      if (b == K) acc[b] += 1.0 - prev;
      cnt[b] += b == bin ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int b = 0; b < KB; ++b)
      if (b <= K) {
        acc[b] += __shfl_xor(acc[b], d, 64);
        cnt[b] += __shfl_xor(cnt[b], d, 64);
      }
    ne += __shfl_xor(ne, d, 64);
  }
  if (lane == 0) {
    const int64_t at = (r * S + s) * (K + 1);
#pragma unroll
    for (int b = 0; b < KB; ++b)
      if (b <= K) { observed[at + b] = cnt[b]; expected[at + b] = acc[b]; }
    empty[r * S + s] = ne;
  }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
struct ed_quant : TotalsMap {         // d_val [2][K][J]: q, below
  int K = 0;
  int64_t tiles_walked = 0, tiles_full = 0;
  DevBuf<int32_t> d_obs;             // [S][E]  the test counts
  DevBuf<int32_t> d_bad;             // [S]  1: shapes outside the model
};

// The quantile map of n_samples samples of the plan's exons at probs [n_probs] (HOST; 1 .. 16, finite, inside (0, 1), strictly
// ascending).  Counts as ed_plan_power_map reads them; phi, expected: HOST arrays [S].  Complete when it returns (it waits for
// `stream`); the counts are not needed afterwards.  The plan must outlive the map.
ED_EXPORT int ed_plan_quantile_map(ed_quant** out, const ed_plan* p, const int32_t* test, const int32_t* ref, int counts_on_device, int layout,
                                   const double* phi, const double* expected, const double* probs, int n_probs, int64_t n_samples, void* stream)
try {
  auto own = [&] {
    switch (edquant::probs_fault(probs, n_probs)) {
      case 0: return (int)ED_OK;
      case 1: return ed_fail(ED_ERR_INVALID, "ed_plan_quantile_map: 1 .. %d probabilities are required", edquant::kMaxProbs);
      case 2: return ed_fail(ED_ERR_INVALID, "ed_plan_quantile_map: a probability is not finite");
      case 3: return ed_fail(ED_ERR_INVALID, "ed_plan_quantile_map: a probability lies outside (0, 1)");
      default: return ed_fail(ED_ERR_INVALID, "ed_plan_quantile_map: the probabilities are not strictly ascending");
    }
  };
  hipStream_t st = (hipStream_t)stream;
  DevBuf<int32_t> up_test, up_ref;
  if (int rc = tm_map_begin("ed_plan_quantile_map", out, p, test, ref, counts_on_device, layout, n_samples, phi, expected, own, up_test, up_ref, st))
    return rc;
  const int64_t S = n_samples, E = p->E, cells = S * E;
  const int K = n_probs;
  std::unique_ptr<ed_quant> h(new ed_quant);
  h->plan = p; h->S = S; h->E = E; h->K = K; h->channels = 2 * K;
  auto nomem = [&](const char* what) { return ed_fail(ED_ERR_NOMEM, "ed_plan_quantile_map: cannot allocate %s", what); };
  std::vector<double> ab;
  std::vector<int32_t> bad;
  h->n_bad = sim_shapes(phi, expected, S, ab, bad);
  DevBuf<double> d_ab, d_probs;
  if (d_ab.alloc((size_t)S * 16) != hipSuccess || d_probs.alloc((size_t)K * 8) != hipSuccess || h->d_bad.alloc((size_t)S * 4) != hipSuccess ||
      h->d_obs.alloc((size_t)std::max<int64_t>(cells, 1) * 4) != hipSuccess)
    return nomem("the samples' parameters and counts");
  HIP_TRY(hipMemcpyAsync(d_ab.get(), ab.data(), (size_t)S * 16, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_probs.get(), probs, (size_t)K * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->d_bad.get(), bad.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));

  PwClock clock;
  PwJobs jobs;
  if (int rc = pw_occupy("ed_plan_quantile_map", *h, jobs, test, ref, layout, st)) return rc;
  if (cells > 0) {
    constexpr int T = edpower::kSlotTile;       // (pw_occupy has refused a grid of more than 65535 sample tiles)
    hipLaunchKernelGGL(k_bq_obs, dim3((unsigned)((E + T - 1) / T), (unsigned)((S + T - 1) / T)), dim3(256), 0, st, test, layout, E, S, h->d_obs.get());
    HIP_TRY(hipGetLastError());
  }
  const int64_t J = h->J;
  const size_t Ja = (size_t)std::max<int64_t>(J, 1);
  DevBuf<int32_t> d_tiles;
  DevBuf<unsigned long long> d_tally;
  if (h->d_val.alloc(Ja * 2 * K * 8) != hipSuccess || d_tiles.alloc(Ja * 4) != hipSuccess || d_tally.alloc(16) != hipSuccess) return nomem("the tables");
  HIP_TRY(hipMemsetAsync(d_tally.get(), 0, 16, st));
  HIP_TRY(hipStreamSynchronize(st));
  h->ms[0] = clock.lap();
  // the walk
  if (J > 0) {
    hipLaunchKernelGGL(k_bq_walk, dim3((unsigned)((J + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, st,
                       (const int32_t*)jobs.d_s.get(), (const int32_t*)jobs.d_n.get(), (const int64_t*)jobs.d_dst.get(), J, (const double*)d_ab.get(),
                       (const int32_t*)h->d_bad.get(), S, (const double*)d_probs.get(), K, h->d_val.get(), d_tiles.get());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  h->ms[1] = clock.lap();
  if (J > 0) {
    hipLaunchKernelGGL(k_bq_tally, dim3(pw_grid(J, 256 * 8)), dim3(256), 0, st, (const int32_t*)jobs.d_n.get(), (const int32_t*)d_tiles.get(), J,
                       d_tally.get());
    HIP_TRY(hipGetLastError());
  }
  unsigned long long tally[2] = {0, 0};
  if (int rc = ed_d2h(tally, d_tally.get(), 16, st)) return rc;
  h->tiles_walked = (int64_t)tally[0];
  h->tiles_full = (int64_t)tally[1];
  *out = h.release();
  return ED_OK;
}
ED_CATCH("ed_plan_quantile_map")

ED_EXPORT void ed_quant_free(ed_quant* qm) { delete qm; }

// Region rows (chrom, start_exon, end_exon of a call row; the other fields are not read) against every sample, to HOST arrays:
// observed [n_rows][S][K + 1], expected [n_rows][S][K + 1], n_empty [n_rows][S].  Every row is checked before anything is enqueued.
ED_EXPORT int ed_quant_regions(ed_quant* qm, const ed_call* rows, int64_t n_rows, int32_t* observed, double* expected, int32_t* n_empty,
                               void* stream)
try {
  hipStream_t st = (hipStream_t)stream;
  DevBuf<ed_call> d_rows;
  if (int rc = tm_regions_begin("ed_quant_regions", qm, rows, n_rows, observed && expected && n_empty, d_rows, st)) return rc;
  if (n_rows == 0) return ED_OK;
  const int64_t R = n_rows, S = qm->S, KB = qm->K + 1;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  DevBuf<double> d_exp;
  DevBuf<int32_t> d_obs, d_empty;
  if (d_exp.alloc((size_t)(R * S * KB) * 8) != hipSuccess || d_obs.alloc((size_t)(R * S * KB) * 4) != hipSuccess ||
      d_empty.alloc((size_t)R * S * 4) != hipSuccess)
    return tm_regions_nomem("ed_quant_regions", R, S);
  PwClock clock;
  hipLaunchKernelGGL(k_bq_regions, dim3((unsigned)(R * sgroups)), dim3(edpower::kRegionWaves * 64), 0, st, (const ed_call*)d_rows.get(), R,
                     (const int32_t*)qm->d_slot.get(), (const int32_t*)qm->d_obs.get(), (const int64_t*)qm->d_tab_off.get(),
                     (const double*)qm->d_val.get(), (const int32_t*)qm->d_bad.get(), qm->J, qm->K, qm->E, S, d_obs.get(), d_exp.get(), d_empty.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  qm->ms[2] = clock.lap();
  HIP_TRY(hipMemcpyAsync(observed, d_obs.get(), (size_t)(R * S * KB) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(expected, d_exp.get(), (size_t)(R * S * KB) * 8, hipMemcpyDeviceToHost, st));
  return ed_d2h(n_empty, d_empty.get(), (size_t)R * S * 4, st);
}
ED_CATCH("ed_quant_regions")

// The per-exon map to a HOST array [2][K][S][E] (q, then below); NaN where the exon's total was skipped, the sample's shapes are outside
// the model or nothing was crossed.  Made in groups of samples through a bounded device buffer.
ED_EXPORT int ed_quant_copy_exons(ed_quant* qm, double* out, void* stream)
try {
  return tm_copy_exons("ed_quant_copy_exons", qm, out, stream);
}
ED_CATCH("ed_quant_copy_exons")

// One sample's table: *n = its occupied totals; when cap >= *n, totals [*n] (ascending) and values [2][K][cap] (q, then below) to HOST arrays
ED_EXPORT int ed_quant_copy_table(const ed_quant* qm, int64_t sample, int32_t* totals, double* values, int64_t cap, int64_t* n)
try {
  return tm_copy_table("ed_quant_copy_table", qm, sample, totals, values, cap, n);
}
ED_CATCH("ed_quant_copy_table")

// counts = ed_power_stats' eight {samples, exons, jobs, most jobs of a sample, cells skipped, samples outside the model, largest valid
// total, words of a map row}, then {probabilities, tiles walked, tiles full walks of the same jobs take}; ms as ed_power_stats
ED_EXPORT int ed_quant_stats(const ed_quant* qm, int64_t counts[11], double ms[4])
try {
  if (!qm || !counts) return ed_fail(ED_ERR_INVALID, "ed_quant_stats: NULL argument");
  tm_stats(*qm, counts, ms);
  counts[8] = qm->K; counts[9] = qm->tiles_walked; counts[10] = qm->tiles_full;
  return ED_OK;
}
ED_CATCH("ed_quant_stats")

// out = ed_power_geometry's four {values of x a walk takes per tile, occupancy cap, largest total walked, exons a region step takes}, then
// the most probabilities of a request
ED_EXPORT int ed_quant_geometry(int32_t out[5])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_quant_geometry: NULL output");
  tm_geometry(out);
  out[4] = edquant::kMaxProbs;
  return ED_OK;
}
ED_CATCH("ed_quant_geometry")

// qbetabinom.ab(p, size, shape1, shape2) (reference R/tools.R:42-53) element by element, HOST arrays of length n: the map's walk with
// one probability, and its bits for the same (size, shapes, p).  NaN: p >= 1 (R's NA), shapes that are not positive and finite, a size
// that is not a whole number in 0 .. the largest total walked (ed_quant_geometry).
ED_EXPORT int ed_qbetabinom_ab(const double* p, const double* size, const double* shape1, const double* shape2, int64_t n, double* out)
try {
  if (n < 0 || n > ((int64_t)1 << 28) || (n > 0 && (!p || !size || !shape1 || !shape2 || !out)))
    return ed_fail(ED_ERR_INVALID, "ed_qbetabinom_ab: bad arguments");
  if (int rc = require_device()) return rc;
  if (n == 0) return ED_OK;
  DevBuf<double> d_in, d_out;
  if (d_in.alloc((size_t)n * 4 * 8) != hipSuccess || d_out.alloc((size_t)n * 2 * 8) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_qbetabinom_ab: cannot allocate %lld elements", (long long)n);
  const double* host[4] = {p, size, shape1, shape2};
  for (int c = 0; c < 4; ++c) HIP_TRY(hipMemcpy(d_in.get() + c * n, host[c], (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_bq_points, dim3((unsigned)((n + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, 0,
                     (const double*)d_in.get(), (const double*)(d_in.get() + n), (const double*)(d_in.get() + 2 * n), (const double*)(d_in.get() + 3 * n), n,
                     d_out.get(), d_out.get() + n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 8, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_qbetabinom_ab")
