// The copy-ratio profile: the summed log-likelihood of the exons of a row (sample, first exon .. last exon) as a function of the copy
// ratio, at up to 16 values per row, straight from the counts (DESIGN.md 4.23).
//
// A row's value at dose mu (-2 < mu <= 2; the copy ratio is 1 + mu / 2) is
//   L(row, mu) = sum over its exons of  lnbeta(a1 + obs_i, (a2 + tot_i) - obs_i) - lnbeta(a1, a2)
//   (a1, a2) = shape_params(ep, sd),  sd = sqrt((phi * e) * (1 - e)),  ep = state_props(e, |mu|)[0] (mu < 0), e (mu = 0), [2] (mu > 0)
// -- the strict emissions of k_emit_rows / k_mix_profile, operation for operation: the term of an exon has the bits the strict mode
// gives the same cell at mixture |mu| in the deletion / normal / duplication column.  The terms are added as a double-double in the one
// order ed_ratio_plan.hpp lays down and rounded once.  On request (the _dd entries) the rounding's remainder is written beside the value:
// L + tail is the double-double sum, so that a difference of two profiles keeps the bits that |L| >> |difference| costs a double.
//
// Geometry (ed_ratio_plan.hpp): one wavefront per item = (row, segment of at most 8 tiles of 64 exons).  Lanes g < G make (a1, a2,
// lnbeta(a1, a2)) of column g once per item.  Every lane loads the counts of its exons of the segment once (parked in LDS words no other
// lane reads) and then takes the columns one after the other -- the column is wave-uniform, so lnbeta's branches mostly are -- adding its
// exons' terms tile by tile.  A segment ends in the fixed tree of a wave reduction; a row of several segments parks the partial sums in
// a workspace and k_ratio_sum adds them in index order.  No atomics.  A lane beyond the segment's last exon loads and evaluates
// nothing: no load leaves the row.
// The bits of a value depend on (the row's counts, phi, expected, mu) alone: the cut into segments follows from the row's length, a
// column's arithmetic does not read G or its own index, idle lanes add (+0, +0), which changes nothing, and nothing is shared between items.

namespace {

// (hi, lo) += (xh, xl): the high words by TwoSum, the low words plainly
__device__ __forceinline__ void dd_merge(double& hi, double& lo, double xh, double xl)
{
  dd_add(hi, lo, xh);
  lo += xl;
}

// what v = hi + lo left of (hi, lo) when it was rounded (TwoSum's error term; 0 beside a value that is not finite)
__device__ __forceinline__ double dd_tail(double hi, double lo, double v)
{
  const double bb = v - hi;
  const double t = (hi - (v - bb)) + (lo - bb);
  return v - v == 0.0 ? t : 0.0;
}

__global__ void __launch_bounds__(edratio::kThreads)
k_ratio_profile(const edratio::Item* __restrict__ items, int64_t n_items, const ed_call* __restrict__ rows, int64_t n_rows,
                const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t ce, int64_t cs, int cb,   // count (e, s) at e * ce + s * cs, cb bytes each
                const double* __restrict__ phi, const double* __restrict__ expected, const double* __restrict__ grid, int G,
                double* __restrict__ ws, double* __restrict__ out, double* __restrict__ tail)   // tail: NULL, or as out
{
  using namespace edratio;
  __shared__ int32_t s_obs[kWaves][kSegExons];
  __shared__ int32_t s_tot[kWaves][kSegExons];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = (int64_t)blockIdx.x * kWaves + wave;
  if (k >= n_items) return;                          // (the whole wave: nothing below is shared between waves)
  const Item it = items[k];
  const int64_t s = rows[it.row].sample;
  const int nt = n_tiles(it.count);
  for (int t = 0; t < nt; ++t) {
    const int i = t * kTile + lane;                   // exon of the segment
    if (i < it.count) {
      const int64_t at = ((int64_t)it.first + i) * ce + s * cs;
      const int32_t obs = ed_ldc(test, at, cb);
      s_obs[wave][i] = obs;
      s_tot[wave][i] = obs + ed_ldc(ref, at, cb);
    }
  }
  // lane g < G: column g of the row
  double a1 = 0.0, a2 = 0.0, c0 = 0.0;
  int ok = 0;
  if (lane < G) {
    const double mu = grid[(int64_t)lane * n_rows + it.row];
    ok = dose_ok(mu) ? 1 : 0;
    const double m = ok ? mu : 0.0;                   // a dose outside the model is evaluated at 0 and reported NaN
    const double ex = expected[s];
    const double sd = __builtin_sqrt((phi[s] * ex) * (1. - ex));
    double ep[3];
    state_props(ex, fabs(m), ep);
    const double e1 = m < 0.0 ? ep[0] : (m > 0.0 ? ep[2] : ep[1]);
    shape_params(e1, sd, a1, a2);
    int f = 0;
    c0 = edsf::lnbeta(a1, a2, &f);
  }
  const double nan = __builtin_nan("");
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    const double b1 = __shfl(a1, g), b2 = __shfl(a2, g), v0 = __shfl(c0, g);
    const int okg = __shfl(ok, g);
    double hi = 0.0, lo = 0.0;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      const int i = t * kTile + lane;
      if (i < it.count) {
        const double obs = (double)s_obs[wave][i], tot = (double)s_tot[wave][i];
        int f1 = 0;
        const double v1 = edsf::lnbeta(b1 + obs, (b2 + tot) - obs, &f1);
        dd_add(hi, lo, v1 - v0);
      }
    }
#pragma unroll
    for (int d = kTile / 2; d >= 1; d >>= 1) {        // p[l] += p[l + d], l < d (the other lanes' sums are not read again)
      const double xh = __shfl_down(hi, d), xl = __shfl_down(lo, d);
      dd_merge(hi, lo, xh, xl);
    }
    if (lane == 0) {
      if (it.slot < 0) {
        const double v = hi + lo;
        out[(int64_t)g * n_rows + it.row] = okg ? v : nan;
        if (tail) tail[(int64_t)g * n_rows + it.row] = okg ? dd_tail(hi, lo, v) : 0.0;
      } else {
        double* w = ws + ((int64_t)it.slot * kMaxGrid + g) * 2;
        w[0] = okg ? hi : nan;
        w[1] = okg ? lo : 0.0;
      }
    }
  }
}

// a row of several segments: segment 0's sum, then the others in index order; one thread per (row, column)
__global__ void k_ratio_sum(const edratio::Multi* __restrict__ multi, int64_t n_multi, int G, int64_t n_rows, const double* __restrict__ ws,
                            double* __restrict__ out, double* __restrict__ tail)
{
  using namespace edratio;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_multi * G) return;
  const Multi m = multi[i / G];
  const int g = (int)(i % G);
  const double* w = ws + ((int64_t)m.slot0 * kMaxGrid + g) * 2;
  double hi = w[0], lo = w[1];
  for (int j = 1; j < m.nseg; ++j) {
    w += kMaxGrid * 2;
    dd_merge(hi, lo, w[0], w[1]);
  }
  const double v = hi + lo;
  out[(int64_t)g * n_rows + m.row] = v;
  if (tail) tail[(int64_t)g * n_rows + m.row] = dd_tail(hi, lo, v);
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// Items of the HOST rows, uploads, the two kernels, the values back; waits for the stream on every way out once something is enqueued
// (the host tables are read by the copies).  d_rows: the rows on the device already (a batch's call table), or NULL.  ev: two events
// recorded around the kernels, or NULL.  tail: HOST [G][n] for the roundings' remainders, or NULL.
static int ratio_run(const ed_call* rows, int64_t n, const ed_call* d_rows, const int32_t* d_test, const int32_t* d_ref, int64_t ce, int64_t cs,
                     int cb, const double* d_phi, const double* d_expected, const double* grid, int G, double* out, double* tail, hipStream_t st,
                     Event* ev)
{
  std::vector<int32_t> first((size_t)n), last((size_t)n);
  for (int64_t r = 0; r < n; ++r) { first[(size_t)r] = rows[r].start_exon; last[(size_t)r] = rows[r].end_exon; }
  edratio::Items plan;
  if (int f = edratio::build_items(first.data(), last.data(), n, plan))
    return ed_fail(ED_ERR_INVALID, f == 1 ? "copy-ratio profile: a row with start > end" : "copy-ratio profile: more than 2^31 - 1 rows or segments");
  const int64_t n_items = (int64_t)plan.items.size(), n_multi = (int64_t)plan.multi.size();
  const size_t cells = (size_t)G * (size_t)n;
  DevBuf<edratio::Item> d_items;
  DevBuf<edratio::Multi> d_multi;
  DevBuf<ed_call> d_own;
  DevBuf<double> d_grid, d_out, d_tail, d_ws;
  if (d_items.alloc((size_t)n_items * sizeof(edratio::Item)) != hipSuccess || d_multi.alloc((size_t)n_multi * sizeof(edratio::Multi)) != hipSuccess ||
      (!d_rows && d_own.alloc((size_t)n * sizeof(ed_call)) != hipSuccess) || d_grid.alloc(cells * 8) != hipSuccess ||
      d_out.alloc(cells * 8) != hipSuccess || (tail && d_tail.alloc(cells * 8) != hipSuccess) || d_ws.alloc((size_t)plan.n_slots * edratio::kMaxGrid * 16) != hipSuccess) {
    (void)hipGetLastError();
    return ed_fail(ED_ERR_NOMEM, "copy-ratio profile: cannot allocate %lld rows x %d values, %lld segments", (long long)n, G, (long long)n_items);
  }
  struct Wait { hipStream_t st; ~Wait() { (void)hipStreamSynchronize(st); } } wait{st};
  HIP_TRY(hipMemcpyAsync(d_items.get(), plan.items.data(), (size_t)n_items * sizeof(edratio::Item), hipMemcpyHostToDevice, st));
  if (n_multi) HIP_TRY(hipMemcpyAsync(d_multi.get(), plan.multi.data(), (size_t)n_multi * sizeof(edratio::Multi), hipMemcpyHostToDevice, st));
  if (!d_rows) {
    HIP_TRY(hipMemcpyAsync(d_own.get(), rows, (size_t)n * sizeof(ed_call), hipMemcpyHostToDevice, st));
    d_rows = d_own.get();
  }
  HIP_TRY(hipMemcpyAsync(d_grid.get(), grid, cells * 8, hipMemcpyHostToDevice, st));
  if (ev) HIP_TRY(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_ratio_profile, dim3((unsigned)((n_items + edratio::kWaves - 1) / edratio::kWaves)), dim3(edratio::kThreads), 0, st,
                     (const edratio::Item*)d_items.get(), n_items, d_rows, n, d_test, d_ref, ce, cs, cb, d_phi, d_expected,
                     (const double*)d_grid.get(), G, d_ws.get(), d_out.get(), d_tail.get());
  HIP_TRY(hipGetLastError());
  if (n_multi) {
    hipLaunchKernelGGL(k_ratio_sum, dim3((unsigned)((n_multi * G + 255) / 256)), dim3(256), 0, st, (const edratio::Multi*)d_multi.get(), n_multi, G,
                       n, (const double*)d_ws.get(), d_out.get(), d_tail.get());
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  if (int rc = ed_d2h(out, d_out.get(), cells * 8, st)) return rc;
  return tail ? ed_d2h(tail, d_tail.get(), cells * 8, st) : ED_OK;
}

static int plan_ratio_profile(const ed_plan* p, const ed_call* rows, int64_t n_rows, const int32_t* d_test, const int32_t* d_ref, int layout,
                              int64_t n_samples, const double* d_phi, const double* d_expected, const double* grid, int G, double* out,
                              double* tail, void* stream)
{
  if (!edratio::grid_ok(G)) return ed_fail(ED_ERR_INVALID, "ed_plan_ratio_profile: G = %d is outside 1 .. %d", G, edratio::kMaxGrid);
  if (!p) return ed_fail(ED_ERR_INVALID, "ed_plan_ratio_profile: NULL plan");
  if (int rc = check_counts_args("ed_plan_ratio_profile", layout, n_samples)) return rc;
  if (n_rows < 0 || n_rows > edratio::kMaxRows) return ed_fail(ED_ERR_INVALID, "ed_plan_ratio_profile: n_rows is outside 0 .. 2^31 - 1");
  if (n_rows > 0 && (!rows || !d_test || !d_ref || !d_phi || !d_expected || !grid || !out)) return ed_fail(ED_ERR_INVALID, "ed_plan_ratio_profile: NULL array");
  if (int rc = check_call_rows("ed_plan_ratio_profile", p, rows, n_rows, n_samples)) return rc;
  if (n_rows == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  const CountStrides cst = count_strides(layout, p->E, n_samples);
  return ratio_run(rows, n_rows, nullptr, d_test, d_ref, cst.ce, cst.cs, 4, d_phi, d_expected, grid, G, out, tail, (hipStream_t)stream, nullptr);
}

ED_EXPORT int ed_plan_ratio_profile(const ed_plan* p, const ed_call* rows, int64_t n_rows, const int32_t* d_test, const int32_t* d_ref, int layout,
                                    int64_t n_samples, const double* d_phi, const double* d_expected, const double* grid, int G, double* out,
                                    void* stream)
try {
  return plan_ratio_profile(p, rows, n_rows, d_test, d_ref, layout, n_samples, d_phi, d_expected, grid, G, out, nullptr, stream);
}
ED_CATCH("ed_plan_ratio_profile")

// ... with the remainder of every value's rounding: out + out_tail is the double-double sum
ED_EXPORT int ed_plan_ratio_profile_dd(const ed_plan* p, const ed_call* rows, int64_t n_rows, const int32_t* d_test, const int32_t* d_ref, int layout,
                                       int64_t n_samples, const double* d_phi, const double* d_expected, const double* grid, int G, double* out,
                                       double* out_tail, void* stream)
try {
  if (n_rows > 0 && !out_tail) return ed_fail(ED_ERR_INVALID, "ed_plan_ratio_profile: NULL array");
  return plan_ratio_profile(p, rows, n_rows, d_test, d_ref, layout, n_samples, d_phi, d_expected, grid, G, out, out_tail, stream);
}
ED_CATCH("ed_plan_ratio_profile_dd")

// The profile of the last run's call table: row i is call i of ed_batch_copy_calls.  Counts, phi and expected are the last run's
// inputs (borrowed: they must still be what the run was given, as for ed_batch_copy_call_info).  A depth-binned or covariate run has no
// single (phi, expected) per sample: refused.  The batch's per-sample mixtures do not enter.
static int batch_call_ratio_profile(ed_batch* b, const double* grid, int G, double* host_out, double* host_tail, bool want_tail, int64_t cap)
{
  if (!edratio::grid_ok(G)) return ed_fail(ED_ERR_INVALID, "ed_batch_copy_call_ratio_profile: G = %d is outside 1 .. %d", G, edratio::kMaxGrid);
  if (b && b->ran && !b->last.plain)
    return ed_fail(ED_ERR_STATE, "ed_batch_copy_call_ratio_profile: the last run was a depth-binned or covariate run, which has no single "
                                 "(phi, expected) per sample; the profile is defined for ed_batch_run only");
  int64_t n = 0;
  if (int rc = ed_batch_n_calls(b, &n)) return rc;   // (grows the table if the run needed more records)
  if (cap < n) return ed_fail(ED_ERR_INVALID, "ed_batch_copy_call_ratio_profile: cap = %lld is below the %lld calls of the run (the grid and the output are [G][calls])",
                              (long long)cap, (long long)n);
  EventSet<2>& ev = b->req.ratio_ev;
  ev.drop();
  if (n <= 0) return ED_OK;
  if (!grid || !host_out || (want_tail && !host_tail)) return ed_fail(ED_ERR_INVALID, "ed_batch_copy_call_ratio_profile: NULL array");
  std::vector<ed_call> rows((size_t)n);
  if (int rc = ed_d2h(rows.data(), b->d_calls, (size_t)n * sizeof(ed_call), b->stream)) return rc;
  const bool timed = b->timing;
  if (timed) HIP_TRY(ev.ready());
  const RunInputs& in = b->last;
  const CountStrides cst = count_strides(in.layout, b->plan->E, b->S);
  if (int rc = ratio_run(rows.data(), n, b->d_calls.get(), in.test, in.ref, cst.ce, cst.cs, in.cb, in.phi, in.expected, grid, G, host_out, host_tail,
                         b->stream, timed ? ev.ev : nullptr))
    return rc;
  ev.live = timed;
  return ED_OK;
}

ED_EXPORT int ed_batch_copy_call_ratio_profile(ed_batch* b, const double* grid, int G, double* host_out, int64_t cap)
try {
  return batch_call_ratio_profile(b, grid, G, host_out, nullptr, false, cap);
}
ED_CATCH("ed_batch_copy_call_ratio_profile")

ED_EXPORT int ed_batch_copy_call_ratio_profile_dd(ed_batch* b, const double* grid, int G, double* host_out, double* host_tail, int64_t cap)
try {
  return batch_call_ratio_profile(b, grid, G, host_out, host_tail, true, cap);
}
ED_CATCH("ed_batch_copy_call_ratio_profile_dd")

// with ed_batch_enable_timing: the time of k_ratio_profile + k_ratio_sum of the last ed_batch_copy_call_ratio_profile of this run, from
// events on its stream; 0 if not timed.  Synchronises that stream.
ED_EXPORT int ed_batch_call_ratio_ms(ed_batch* b, float* ms)
try {
  if (!b || !ms) return ed_fail(ED_ERR_INVALID, "NULL argument");
  return request_ms(b, b->req.ratio_ev, 0, 1, ms);
}
ED_CATCH("ed_batch_call_ratio_ms")

// out = {tiles of 64 exons a segment holds, exons up to which a row takes the narrow mapping (0: there is none), grid points a launch takes,
// items a workgroup serves}: what a test needs to place its rows on the edges
ED_EXPORT int ed_ratio_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_ratio_geometry: NULL output");
  out[0] = edratio::kSegTiles; out[1] = edratio::kNarrow; out[2] = edratio::kMaxGrid; out[3] = edratio::kWaves;
  return ED_OK;
}
ED_CATCH("ed_ratio_geometry")
