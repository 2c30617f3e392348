// Draws from the fitted model: rbetabinom, and a whole cohort's counts redrawn under its own fitted normal state, conditional on every
// cell's total as the model itself conditions (DESIGN.md 4.26).
//
// For a size n, shapes (a, b) and a uniform u: pm[x] = the beta-binomial mass at x = 0 .. n, C(x) = pm[0] + .. + pm[x],
//   the draw = the smallest x in 0 .. n with C(x) > u;   n when nothing crosses (u within rounding of 1);   0 for n = 0
// -- inversion of the distribution function, qbetabinom's `cut` (edquant.inc) at p = u.  The uniform is ed_philox.hpp's: Philox4x32-10 at
// the counter (exon, global sample, replicate, stream) under the key of a 64-bit seed.  Sample s has a = expected (1 - phi) / phi,
// b = (1 - expected)(1 - phi) / phi in qbetabinom's own operation order, formed on the host by the function the quantile map forms them
// with (edtotals.inc: sim_shapes).
//
// The walk (sim_walk) takes C from the CDF walk of edtotals.inc (bb_open, bb_step), the code bq_walk takes it from: C here and C there
// are the same operations because they are the same source.  It locates a uniform with bq_walk's comparisons (incl > u, then
// excl + part[t] > u).  What differs is how many uniforms one walk serves: the lanes hold up to 64 of them, after each tile every
// pending uniform the tile can cross is made wave-uniform in turn and located, and the walk ends with the tile in which the last one
// was crossed.  C does not depend on the uniforms, and a uniform is compared with C alone: the bits of a draw depend on (n, a, b, u) --
// not on the other uniforms of the walk, their number or their lanes.  The element-wise kernel is the same function with one uniform in
// lane 0.
// The cohort draw walks every sample once per OCCUPIED total (edtotals.inc's occupancy, job list and slots, as they are), longest first,
// and serves all cells of that (sample, total) from the one walk, 64 at a time.  A job's cells are the inverse of the slot map: count
// (integer atomics) -> exclusive scan (edannot.inc's) -> fill (an integer cursor per job).  The order in which a job's cells are listed
// varies from run to run; a cell's draw does not depend on its place in the list.  No atomics on doubles anywhere in this file.

namespace edsim {
constexpr int kChunk = 64;                    // uniforms one walk holds
constexpr int64_t kMaxPoints = (int64_t)1 << 28;
// 0: fine; 1: the two ranges of `bytes` bytes overlap
inline int ranges_overlap(const void* a, const void* b, size_t bytes)
{
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return (x < y + bytes && y < x + bytes) ? 1 : 0;
}
struct Stats {
  int64_t counts[6] = {0, 0, 0, 0, 0, 0};     // jobs, tiles walked, tiles of full walks, cells drawn, cells skipped, samples outside the model
  double ms[3] = {0, 0, 0};                   // occupancy, grouping, walk
};
}  // namespace edsim

namespace {

// One wavefront: lane l < cnt holds the uniform u (0 <= u < 1); the lane's draw from BetaBinomial(n, a, b) is returned in that lane.
// `tiles` goes up by the tiles walked.
__device__ __forceinline__ int32_t sim_walk(int64_t n, double a, double b, double u, int cnt, int lane, int32_t& tiles)
{
  constexpr int P = edpower::kWalkPer;
  if (n == 0) return 0;
  bool pending = lane < cnt;
  int32_t x = (int32_t)n;                     // nothing crosses: n
  BbWalk w = bb_open(n, a, b, lane);
  const int64_t nt = edpower::n_walk_tiles(n);
  for (int64_t tile = 0; tile < nt && __ballot(pending); ++tile) {
    ++tiles;
    const BbTile c = bb_step(w, tile, lane);
    // the largest C any lane of the tile ends on: some lane has incl > u exactly when this has
    double top = c.holds ? c.incl : -1.0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) top = __builtin_fmax(top, __shfl_xor(top, d, 64));
    unsigned long long todo = __ballot(pending && top > u);
    while (todo) {
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const double uk = __shfl(u, k, 64);
      const unsigned long long hit = __ballot(c.holds && c.incl > uk);
      if (!hit) continue;
      const int first = __ffsll((long long)hit) - 1;
      int32_t xv = 0;
      if (lane == first) {
        // the first of the four whose C exceeds uk: the last does
        int j = P - 1;
#pragma unroll
        for (int t = P - 2; t >= 0; --t)
          if (c.excl + c.part[t] > uk) j = t;
        const int64_t v = c.xs + j;
        xv = (int32_t)(v < n ? v : n);
      }
      const int32_t got = __shfl(xv, first, 64);
      if (lane == k) { x = got; pending = false; }
    }
  }
  return x;
}

__global__ void __launch_bounds__(256)
k_sim_unif(uint64_t seed, const uint32_t* __restrict__ exon, const uint32_t* __restrict__ sample, const uint32_t* __restrict__ replicate,
           uint32_t stream_id, int64_t N, double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) out[i] = edphilox::u53(seed, exon[i], sample[i], replicate[i], stream_id);
}

__device__ __forceinline__ bool sim_shapes_ok(double sa, double sb) { return sa > 0.0 && sb > 0.0 && sa < HUGE_VAL && sb < HUGE_VAL; }

// the element-wise form: a wavefront per (u, size, a, b); -1 where the uniform is outside [0, 1), the shapes are not positive and finite
// or the size is not a whole number in 0 .. the largest total walked
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_sim_points(const double* __restrict__ u, const double* __restrict__ size, const double* __restrict__ a, const double* __restrict__ b, int64_t N,
             int32_t* __restrict__ x)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * edpower::kWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= N) return;
  const double su = u[i], sz = size[i], sa = a[i], sb = b[i];
  const bool ok = su >= 0.0 && su < 1.0 && sim_shapes_ok(sa, sb) && sz >= 0.0 && sz <= (double)edpower::kMaxTotal && (double)(int64_t)sz == sz;
  if (!ok) {
    if (lane == 0) x[i] = -1;
    return;
  }
  int32_t tiles = 0;
  const int32_t v = sim_walk((int64_t)sz, sa, sb, su, 1, lane, tiles);
  if (lane == 0) x[i] = v;
}

// listed cells of a cohort, a wavefront per cell: the cell's total from the counts, its own shapes, the uniform of `stream_id`.  A cell
// whose total is not walked or whose shapes are outside the model keeps what the outputs hold.
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_sim_cells(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const int32_t* __restrict__ cell_e, const int32_t* __restrict__ cell_s,
            const double* __restrict__ a, const double* __restrict__ b, int64_t N, int layout, int64_t E, int64_t S, uint64_t seed, uint32_t sample0,
            uint32_t replicate, uint32_t stream_id, int32_t* __restrict__ test_out, int32_t* __restrict__ ref_out)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * edpower::kWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= N) return;
  const int64_t e = cell_e[i], s = cell_s[i];
  const int64_t at = layout ? s * E + e : e * S + s;
  const int64_t n = pw_total(test, ref, at);
  const double sa = a[i], sb = b[i];
  if (!edpower::total_ok(n) || !sim_shapes_ok(sa, sb)) return;
  const double u = edphilox::u53(seed, (uint32_t)e, sample0 + (uint32_t)s, replicate, stream_id);
  int32_t tiles = 0;
  const int32_t v = sim_walk(n, sa, sb, u, 1, lane, tiles);
  if (lane == 0) { test_out[at] = v; ref_out[at] = (int32_t)n - v; }
}

// ---- a job's cells: the inverse of the slot map --------------------------------------------------------------------------------
// cnt[t] = the cells whose total stands at place t of the tables (t = tab_off[s] + slot)
__global__ void __launch_bounds__(256)
k_sim_count(const int32_t* __restrict__ slot, const int64_t* __restrict__ tab_off, int64_t E, int64_t cells, unsigned long long* __restrict__ cnt)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int32_t sl = slot[i];
    if (sl >= 0) atomicAdd(cnt + tab_off[i / E] + sl, 1ull);
  }
}

// list[off[t] .. off[t + 1]) = the exons of place t, in the order the cursor hands the places out
__global__ void __launch_bounds__(256)
k_sim_fill(const int32_t* __restrict__ slot, const int64_t* __restrict__ tab_off, const int64_t* __restrict__ off, int64_t E, int64_t cells,
           unsigned int* __restrict__ cursor, int32_t* __restrict__ list)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int32_t sl = slot[i];
    if (sl < 0) continue;
    const int64_t t = tab_off[i / E] + sl;
    const int64_t at = off[t] + (int64_t)atomicAdd(cursor + t, 1u);
    if (at < off[t + 1]) list[at] = (int32_t)(i % E);              // (the cursor stays inside the count of the same cells)
  }
}

// ---- the cohort walk -----------------------------------------------------------------------------------------------------------
// One wavefront per occupied (sample, total), longest first; the job's cells 64 at a time, one walk per 64.  ab [2][S]; tiles [J]
__global__ void __launch_bounds__(edpower::kWalkWaves * 64)
k_sim_walk(const int32_t* __restrict__ job_s, const int32_t* __restrict__ job_n, const int64_t* __restrict__ job_dst, int64_t J,
           const int64_t* __restrict__ off, const int32_t* __restrict__ list, const double* __restrict__ ab, const int32_t* __restrict__ bad,
           int layout, int64_t E, int64_t S, uint64_t seed, uint32_t sample0, uint32_t replicate, int32_t* __restrict__ test_out,
           int32_t* __restrict__ ref_out, int32_t* __restrict__ tiles)
{
  const int lane = threadIdx.x & 63;
  const int64_t jb = (int64_t)blockIdx.x * edpower::kWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (jb >= J) return;
  const int64_t s = job_s[jb], dst = job_dst[jb];
  const int64_t n = job_n[jb];
  if (bad[s]) {
    if (lane == 0) tiles[jb] = 0;
    return;
  }
  const double a = ab[s], b = ab[S + s];
  const int64_t lo = off[dst], hi = off[dst + 1];
  int32_t t = 0;
  for (int64_t c0 = lo; c0 < hi; c0 += edsim::kChunk) {
    const int cnt = (int)(hi - c0 < edsim::kChunk ? hi - c0 : edsim::kChunk);
    int64_t e = 0;
    double u = 0.0;
    if (lane < cnt) {
      e = list[c0 + lane];
      u = edphilox::u53(seed, (uint32_t)e, sample0 + (uint32_t)s, replicate, edphilox::kStreamNull);
    }
    const int32_t v = sim_walk(n, a, b, u, cnt, lane, t);
    if (lane < cnt) {
      const int64_t at = layout ? s * E + e : e * S + s;
      test_out[at] = v;
      ref_out[at] = (int32_t)n - v;
    }
  }
  if (lane == 0) tiles[jb] = t;
}

// out [3]: the tiles walked, the tiles that one full walk per 64 cells of the same jobs takes, the cells drawn
__global__ void __launch_bounds__(256)
k_sim_tally(const int32_t* __restrict__ job_s, const int32_t* __restrict__ job_n, const int64_t* __restrict__ job_dst,
            const int32_t* __restrict__ tiles, const int64_t* __restrict__ off, const int32_t* __restrict__ bad, int64_t J,
            unsigned long long* __restrict__ out)
{
  unsigned long long walked = 0, full = 0, drawn = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < J; i += (int64_t)gridDim.x * 256) {
    if (bad[job_s[i]]) continue;
    const int64_t dst = job_dst[i], len = off[dst + 1] - off[dst];
    walked += (unsigned long long)tiles[i];
    if (job_n[i] > 0) full += (unsigned long long)(edpower::n_walk_tiles(job_n[i]) * ((len + edsim::kChunk - 1) / edsim::kChunk));
    drawn += (unsigned long long)len;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    walked += __shfl_xor(walked, d, 64);
    full += __shfl_xor(full, d, 64);
    drawn += __shfl_xor(drawn, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, walked);
    atomicAdd(out + 1, full);
    atomicAdd(out + 2, drawn);
  }
}

thread_local edsim::Stats g_sim_stats;      // of the calling thread's last ed_plan_simulate

// what ed_plan_simulate and ed_plan_simulate_cells refuse alike, before anything is enqueued
int sim_check(const char* entry, const ed_plan* p, const int32_t* test, const int32_t* ref, int64_t n_samples, int64_t sample0, int layout,
              int64_t replicate, const int32_t* test_out, const int32_t* ref_out)
{
  if (!p) return ed_fail(ED_ERR_INVALID, "%s: NULL plan", entry);
  if (int rc = check_counts_args(entry, layout, n_samples)) return rc;
  if (p->E > 0 && (!test || !ref || !test_out || !ref_out)) return ed_fail(ED_ERR_INVALID, "%s: NULL array", entry);
  if (replicate < 0 || replicate > 0xffffffffLL) return ed_fail(ED_ERR_INVALID, "%s: replicate is outside 0 .. 2^32 - 1", entry);
  if (sample0 < 0 || sample0 + n_samples > ((int64_t)1 << 32)) return ed_fail(ED_ERR_INVALID, "%s: sample0 .. sample0 + n_samples leaves 0 .. 2^32", entry);
  const size_t bytes = (size_t)(p->E * n_samples) * 4;
  if (bytes > 0 && (edsim::ranges_overlap(test_out, test, bytes) || edsim::ranges_overlap(test_out, ref, bytes) ||
                    edsim::ranges_overlap(ref_out, test, bytes) || edsim::ranges_overlap(ref_out, ref, bytes) ||
                    edsim::ranges_overlap(test_out, ref_out, bytes)))
    return ed_fail(ED_ERR_INVALID, "%s: the outputs may not alias the counts or each other", entry);
  return ED_OK;
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// u [n] (HOST) = the uniforms of the counters (exon[i], sample[i], replicate[i], stream_id) under `seed` (HOST uint32 arrays), made on
// the device by the code the draws use
ED_EXPORT int ed_runif53(uint64_t seed, const uint32_t* exon, const uint32_t* sample, const uint32_t* replicate, uint32_t stream_id, int64_t n,
                         double* u_out)
try {
  if (n < 0 || n > edsim::kMaxPoints || (n > 0 && (!exon || !sample || !replicate || !u_out))) return ed_fail(ED_ERR_INVALID, "ed_runif53: bad arguments");
  if (int rc = require_device()) return rc;
  if (n == 0) return ED_OK;
  DevBuf<uint32_t> d_in;
  DevBuf<double> d_out;
  if (d_in.alloc((size_t)n * 3 * 4) != hipSuccess || d_out.alloc((size_t)n * 8) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_runif53: cannot allocate %lld elements", (long long)n);
  const uint32_t* host[3] = {exon, sample, replicate};
  for (int c = 0; c < 3; ++c) HIP_TRY(hipMemcpy(d_in.get() + c * n, host[c], (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_sim_unif, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, seed, (const uint32_t*)d_in.get(), (const uint32_t*)(d_in.get() + n),
                     (const uint32_t*)(d_in.get() + 2 * n), stream_id, n, d_out.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(u_out, d_out.get(), (size_t)n * 8, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_runif53")

// x [n] (HOST int32) = the draw from BetaBinomial(size[i], a[i], b[i]) at the uniform u[i], element by element over HOST arrays: the
// cohort draw's walk with one uniform, and its bits for the same (size, shapes, u).  -1: u outside [0, 1), shapes that are not positive
// and finite, a size that is not a whole number in 0 .. the largest total walked.
ED_EXPORT int ed_rbetabinom_ab_u(const double* u, const double* size, const double* a, const double* b, int64_t n, int32_t* x_out)
try {
  if (n < 0 || n > edsim::kMaxPoints || (n > 0 && (!u || !size || !a || !b || !x_out))) return ed_fail(ED_ERR_INVALID, "ed_rbetabinom_ab_u: bad arguments");
  if (int rc = require_device()) return rc;
  if (n == 0) return ED_OK;
  DevBuf<double> d_in;
  DevBuf<int32_t> d_out;
  if (d_in.alloc((size_t)n * 4 * 8) != hipSuccess || d_out.alloc((size_t)n * 4) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_rbetabinom_ab_u: cannot allocate %lld elements", (long long)n);
  const double* host[4] = {u, size, a, b};
  for (int c = 0; c < 4; ++c) HIP_TRY(hipMemcpy(d_in.get() + c * n, host[c], (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_sim_points, dim3((unsigned)((n + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, 0,
                     (const double*)d_in.get(), (const double*)(d_in.get() + n), (const double*)(d_in.get() + 2 * n), (const double*)(d_in.get() + 3 * n), n,
                     d_out.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(x_out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_rbetabinom_ab_u")

// The cohort draw.  test / ref, test_out / ref_out: DEVICE int32 counts of n_samples samples of the plan's exons in `layout`; phi,
// expected: HOST arrays [n_samples].  Every cell: n = test + ref, test_out = the draw at u(seed, exon, sample0 + s, replicate, 0) under
// its sample's shapes, ref_out = n - test_out.  A cell whose total the occupancy map skips, and every cell of a sample whose shapes are
// outside the model, keeps its input counts and is tallied (ed_sim_stats).  Complete when it returns (it waits for `stream`).
ED_EXPORT int ed_plan_simulate(const ed_plan* p, const int32_t* test, const int32_t* ref, const double* phi, const double* expected,
                               int64_t n_samples, int64_t sample0, int layout, uint64_t seed, int64_t replicate, int32_t* test_out,
                               int32_t* ref_out, void* stream)
try {
  if (int rc = sim_check("ed_plan_simulate", p, test, ref, n_samples, sample0, layout, replicate, test_out, ref_out)) return rc;
  if (!phi || !expected) return ed_fail(ED_ERR_INVALID, "ed_plan_simulate: NULL array");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = n_samples, E = p->E, cells = S * E;
  edsim::Stats stats;
  auto nomem = [&](const char* what) { return ed_fail(ED_ERR_NOMEM, "ed_plan_simulate: cannot allocate %s", what); };
  std::vector<double> ab;
  std::vector<int32_t> bad;
  stats.counts[5] = sim_shapes(phi, expected, S, ab, bad);
  if (cells == 0) { g_sim_stats = stats; return ED_OK; }
  DevBuf<double> d_ab;
  DevBuf<int32_t> d_bad;
  if (d_ab.alloc((size_t)S * 16) != hipSuccess || d_bad.alloc((size_t)S * 4) != hipSuccess) return nomem("the samples' parameters");
  HIP_TRY(hipMemcpyAsync(d_ab.get(), ab.data(), (size_t)S * 16, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_bad.get(), bad.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
  // every cell starts as its input: the walk overwrites the ones it draws
  HIP_TRY(hipMemcpyAsync(test_out, test, (size_t)cells * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(ref_out, ref, (size_t)cells * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));

  PwClock clock;
  PwOccupancy occ;
  occ.S = S; occ.E = E;
  PwJobs jobs;
  if (int rc = pw_occupy("ed_plan_simulate", occ, jobs, test, ref, layout, st)) return rc;
  stats.ms[0] = clock.lap();
  const int64_t J = occ.J;
  stats.counts[0] = J;
  if (J == 0) {
    stats.counts[4] = cells;
    g_sim_stats = stats;
    return ED_OK;
  }
  // the jobs' cells
  const int64_t nb = (J + kAnnotScanBlock - 1) / kAnnotScanBlock;
  DevBuf<unsigned long long> d_cnt, d_tally;
  DevBuf<int64_t> d_off, d_bsum;
  DevBuf<unsigned int> d_cursor;
  DevBuf<int32_t> d_list, d_tiles;
  if (d_cnt.alloc((size_t)J * 8) != hipSuccess || d_off.alloc((size_t)(J + 1) * 8) != hipSuccess || d_bsum.alloc((size_t)nb * 8) != hipSuccess ||
      d_cursor.alloc((size_t)J * 4) != hipSuccess || d_list.alloc((size_t)cells * 4) != hipSuccess || d_tiles.alloc((size_t)J * 4) != hipSuccess ||
      d_tally.alloc(24) != hipSuccess)
    return nomem("the jobs' cells");
  HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, (size_t)J * 8, st));
  HIP_TRY(hipMemsetAsync(d_cursor.get(), 0, (size_t)J * 4, st));
  HIP_TRY(hipMemsetAsync(d_tally.get(), 0, 24, st));
  hipLaunchKernelGGL(k_sim_count, dim3(pw_grid(cells, 256 * 8)), dim3(256), 0, st, (const int32_t*)occ.d_slot.get(), (const int64_t*)occ.d_tab_off.get(), E,
                     cells, d_cnt.get());
  hipLaunchKernelGGL(k_annot_scan_block, dim3((unsigned)nb), dim3(kAnnotBlock), 0, st, (const int64_t*)d_cnt.get(), J, d_off.get(), d_bsum.get());
  hipLaunchKernelGGL(k_annot_scan_sums, dim3(1), dim3(1024), 0, st, d_bsum.get(), nb, d_off.get() + J);
  hipLaunchKernelGGL(k_annot_scan_add, dim3((unsigned)nb), dim3(kAnnotBlock), 0, st, d_off.get(), J, (const int64_t*)d_bsum.get());
  hipLaunchKernelGGL(k_sim_fill, dim3(pw_grid(cells, 256 * 8)), dim3(256), 0, st, (const int32_t*)occ.d_slot.get(), (const int64_t*)occ.d_tab_off.get(),
                     (const int64_t*)d_off.get(), E, cells, d_cursor.get(), d_list.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  stats.ms[1] = clock.lap();
  // the walk
  hipLaunchKernelGGL(k_sim_walk, dim3((unsigned)((J + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, st,
                     (const int32_t*)jobs.d_s.get(), (const int32_t*)jobs.d_n.get(), (const int64_t*)jobs.d_dst.get(), J, (const int64_t*)d_off.get(),
                     (const int32_t*)d_list.get(), (const double*)d_ab.get(), (const int32_t*)d_bad.get(), layout, E, S, seed, (uint32_t)sample0,
                     (uint32_t)replicate, test_out, ref_out, d_tiles.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  stats.ms[2] = clock.lap();
  hipLaunchKernelGGL(k_sim_tally, dim3(pw_grid(J, 256 * 8)), dim3(256), 0, st, (const int32_t*)jobs.d_s.get(), (const int32_t*)jobs.d_n.get(),
                     (const int64_t*)jobs.d_dst.get(), (const int32_t*)d_tiles.get(), (const int64_t*)d_off.get(), (const int32_t*)d_bad.get(), J,
                     d_tally.get());
  HIP_TRY(hipGetLastError());
  unsigned long long tally[3] = {0, 0, 0};
  if (int rc = ed_d2h(tally, d_tally.get(), 24, st)) return rc;
  stats.counts[1] = (int64_t)tally[0];
  stats.counts[2] = (int64_t)tally[1];
  stats.counts[3] = (int64_t)tally[2];
  stats.counts[4] = cells - (int64_t)tally[2];
  g_sim_stats = stats;
  return ED_OK;
}
ED_CATCH("ed_plan_simulate")

// Listed cells of the same cohort redrawn under shapes of their own (planted cells: the null draw's cells under a shifted proportion).
// cell_exon, cell_sample (the sample's index in this slab), a, b: HOST arrays [n_cells]; the total of a cell is read from test / ref
// (DEVICE, the counts ed_plan_simulate read), its uniform is u(seed, exon, sample0 + sample, replicate, stream_id), and the draw
// overwrites the cell in test_out / ref_out (DEVICE).  A cell whose total is not walked or whose shapes are not positive and finite is
// left as it is.  Every cell is checked against the plan and n_samples before anything is enqueued.  Complete when it returns.
ED_EXPORT int ed_plan_simulate_cells(const ed_plan* p, const int32_t* test, const int32_t* ref, const int32_t* cell_exon, const int32_t* cell_sample,
                                     const double* a, const double* b, int64_t n_cells, int64_t n_samples, int64_t sample0, int layout, uint64_t seed,
                                     int64_t replicate, uint32_t stream_id, int32_t* test_out, int32_t* ref_out, void* stream)
try {
  if (int rc = sim_check("ed_plan_simulate_cells", p, test, ref, n_samples, sample0, layout, replicate, test_out, ref_out)) return rc;
  if (n_cells < 0 || n_cells > edsim::kMaxPoints) return ed_fail(ED_ERR_INVALID, "ed_plan_simulate_cells: n_cells is outside 0 .. 2^28");
  if (n_cells > 0 && (!cell_exon || !cell_sample || !a || !b)) return ed_fail(ED_ERR_INVALID, "ed_plan_simulate_cells: NULL array");
  for (int64_t i = 0; i < n_cells; ++i)
    if (cell_exon[i] < 0 || cell_exon[i] >= p->E || cell_sample[i] < 0 || cell_sample[i] >= n_samples)
      return ed_fail(ED_ERR_INVALID, "ed_plan_simulate_cells: cell %lld lies outside the counts", (long long)i);
  if (n_cells == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = n_cells;
  DevBuf<int32_t> d_idx;
  DevBuf<double> d_ab;
  if (d_idx.alloc((size_t)N * 8) != hipSuccess || d_ab.alloc((size_t)N * 16) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_plan_simulate_cells: cannot allocate %lld cells", (long long)N);
  HIP_TRY(hipMemcpyAsync(d_idx.get(), cell_exon, (size_t)N * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_idx.get() + N, cell_sample, (size_t)N * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_ab.get(), a, (size_t)N * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_ab.get() + N, b, (size_t)N * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sim_cells, dim3((unsigned)((N + edpower::kWalkWaves - 1) / edpower::kWalkWaves)), dim3(edpower::kWalkWaves * 64), 0, st, test, ref,
                     (const int32_t*)d_idx.get(), (const int32_t*)(d_idx.get() + N), (const double*)d_ab.get(), (const double*)(d_ab.get() + N), N, layout,
                     p->E, n_samples, seed, (uint32_t)sample0, (uint32_t)replicate, stream_id, test_out, ref_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return ED_OK;
}
ED_CATCH("ed_plan_simulate_cells")

// of the calling thread's last ed_plan_simulate: counts = {jobs, tiles walked, tiles that one full walk per 64 cells of the same jobs
// takes, cells drawn, cells skipped, samples outside the model}; ms (may be NULL) = {occupancy, grouping, walk}, host-timed between waits
ED_EXPORT int ed_sim_stats(int64_t counts[6], double ms[3])
try {
  if (!counts) return ed_fail(ED_ERR_INVALID, "ed_sim_stats: NULL argument");
  for (int i = 0; i < 6; ++i) counts[i] = g_sim_stats.counts[i];
  if (ms) for (int i = 0; i < 3; ++i) ms[i] = g_sim_stats.ms[i];
  return ED_OK;
}
ED_CATCH("ed_sim_stats")

// out = ed_power_geometry's four {values of x a walk takes per tile, occupancy cap, largest total walked, exons a region step takes}, then
// the uniforms one walk holds
ED_EXPORT int ed_sim_geometry(int32_t out[5])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_sim_geometry: NULL output");
  tm_geometry(out);
  out[4] = edsim::kChunk;
  return ED_OK;
}
ED_CATCH("ed_sim_geometry")
