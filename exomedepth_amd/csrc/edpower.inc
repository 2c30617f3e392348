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
struct ed_power : TotalsMap {};      // d_val [4][J]: mean_del, var_del, mean_dup, var_dup

// The map of n_samples samples of the plan's exons.  test / ref: int32 counts, [E][S] (layout 0) or [S][E] (layout 1), on the device
// (counts_on_device != 0) or on the host; phi, expected, mixture_s: HOST arrays [S]; mixture_s NULL: `mixture` for every sample.
// Complete when it returns (it waits for `stream`); the counts are not needed afterwards.  The plan must outlive the map.
ED_EXPORT int ed_plan_power_map(ed_power** out, const ed_plan* p, const int32_t* test, const int32_t* ref, int counts_on_device, int layout,
                                int64_t n_samples, const double* phi, const double* expected, const double* mixture_s, double mixture,
                                void* stream)
try {
  hipStream_t st = (hipStream_t)stream;
  DevBuf<int32_t> up_test, up_ref;
  if (int rc = tm_map_begin("ed_plan_power_map", out, p, test, ref, counts_on_device, layout, n_samples, phi, expected, [] { return ED_OK; },
                            up_test, up_ref, st))
    return rc;
  const int64_t S = n_samples, E = p->E;
  std::unique_ptr<ed_power> h(new ed_power);
  h->plan = p; h->S = S; h->E = E; h->channels = 4;
  auto nomem = [&](const char* what) { return ed_fail(ED_ERR_NOMEM, "ed_plan_power_map: cannot allocate %s", what); };
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
  hipStream_t st = (hipStream_t)stream;
  DevBuf<ed_call> d_rows;
  if (int rc = tm_regions_begin("ed_power_regions", pm, rows, n_rows, sums && n_empty && price && n_exons, d_rows, st)) return rc;
  if (n_rows == 0) return ED_OK;
  const ed_plan* p = pm->plan;
  const int64_t R = n_rows, S = pm->S;
  const int64_t sgroups = (S + edpower::kRegionWaves - 1) / edpower::kRegionWaves;
  DevBuf<double> d_sums, d_price;
  DevBuf<int32_t> d_empty;
  if (d_sums.alloc((size_t)R * S * 4 * 8) != hipSuccess || d_price.alloc((size_t)R * 8) != hipSuccess || d_empty.alloc((size_t)R * S * 4) != hipSuccess)
    return tm_regions_nomem("ed_power_regions", R, S);
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
  return tm_copy_exons("ed_power_copy_exons", pm, out, stream);
}
ED_CATCH("ed_power_copy_exons")

// One sample's table: *n = its occupied totals; when cap >= *n, totals [*n] (ascending) and values [4][cap] to HOST arrays
ED_EXPORT int ed_power_copy_table(const ed_power* pm, int64_t sample, int32_t* totals, double* values, int64_t cap, int64_t* n)
try {
  return tm_copy_table("ed_power_copy_table", pm, sample, totals, values, cap, n);
}
ED_CATCH("ed_power_copy_table")

// counts = {samples, exons, jobs, most jobs of a sample, cells skipped, samples outside the model, largest valid total, words of a map row};
// ms = {occupancy, walk, kernels of the last ed_power_regions, kernels of the last ed_power_copy_exons}, host-timed between waits
ED_EXPORT int ed_power_stats(const ed_power* pm, int64_t counts[8], double ms[4])
try {
  if (!pm || !counts) return ed_fail(ED_ERR_INVALID, "ed_power_stats: NULL argument");
  tm_stats(*pm, counts, ms);
  return ED_OK;
}
ED_CATCH("ed_power_stats")

// out = {values of x a walk takes per tile, occupancy cap, largest total walked, exons a region step takes}
ED_EXPORT int ed_power_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_power_geometry: NULL output");
  tm_geometry(out);
  return ED_OK;
}
ED_CATCH("ed_power_geometry")
