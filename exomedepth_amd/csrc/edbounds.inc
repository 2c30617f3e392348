// Breakpoint credible intervals of call rows, from the posterior of edpost.inc (DESIGN.md 4.20).
//
// A row of type T lies in a chain lo .. hi-1.  Its anchor a is the exon of the row with the largest log gamma(T) (ties to the lowest
// index, NaN ignored).  With w_t = B_t + e_t(T) -- B_t the stay entry of exon t's gap, read as k_call_post reads it -- the extent of the
// run of T through the anchor is
//   G_L(i) = ((log gamma_i(T) - beta_i(T)) + (beta_a(T) - log gamma_a(T))) + sum_{t=i+1..a} w_t        i <= a
//   G_R(j) = (beta_j(T) - beta_a(T)) + sum_{t=a+1..j} w_t                                             j >= a
// (log_p_all's identity, walked outward; G(a) = 0).  exp G_L(i) = P(left edge of the run <= i | x_a = T), and the same to the right.
// Walking outward from the anchor, a bound is the last exon before the FIRST one whose G is below the threshold (or is NaN, or lies
// outside the chain): log1p(-tail) for start_hi / end_lo, log(tail) for start_lo / end_hi.  In floating point G is not monotone where
// gamma is 1 to the last bit, hence first failure and no search.
//
// Geometry: one wavefront per row.  A walk takes a tile of 64 consecutive exons per step: lane l of the tile at distance `base` holds the
// exon at distance k = base + l from the anchor, the four strided loads of the 64 lanes (e, B, beta, and log gamma on the left walk) in
// flight together -- a thread per row pays one dependent round trip per exon, which is what a whole-chromosome row (19 352 exons) cannot
// afford.  The running sum is a 6-step inclusive wave scan in plain double; the carry into the next tile is the last lane's value, added
// into a double-double (dd_add), so that a sum's error does not grow with the length of the walk.  A ballot of G >= threshold and a
// find-first on its complement give both crossings; most walks end inside the first tile.  From the second tile on the next tile's loads
// are issued before the current tile's scan.  Lanes beyond the chain load the chain's edge exon and fail every threshold, so no load
// leaves the chain.  One operation order per row, no atomics, nothing shared between rows: a row's values depend on the row alone.

namespace {

// larger value wins, equal values the lower exon; a NaN never wins (the comparisons are false) and never holds (it is not put in)
__device__ __forceinline__ void bounds_argmax(double& v, int& ix, double ov, int oi)
{
  const bool take = ov > v || (ov == v && oi < ix);
  v = take ? ov : v;
  ix = take ? oi : ix;
}

struct BoundsTile { double e, B, b, lg; };

// dir = -1: towards the chain's first exon, +1: towards its last.  kmax: the distance of the chain's edge, kneed: of the row's own edge
// (<= kmax).  Leaves the distances of the two bounds and G at the row's edge.  Everything but `lane` is wave-uniform.
template <int dir>
__device__ __forceinline__ void bounds_walk(int lane, int64_t a, int kmax, int kneed, const double* __restrict__ ecol, int64_t le,
                                            const double* __restrict__ Bp, const double* __restrict__ bcol, const double* __restrict__ gcol,
                                            int64_t S, double head_a, double thi, double tlo, int& k_in, int& k_out, double& keep)
{
  auto load = [&](int base) {
    const int kr = base + lane;
    const int k = kr < kmax ? kr : kmax;                       // beyond the chain: its edge exon again
    const int64_t x = a + (int64_t)dir * k;
    const int64_t xw = (dir < 0 && k > 0) ? x + 1 : x;         // the step that joins distance k - 1 to k: exon x + 1 (left), x (right)
    BoundsTile t;
    t.e = ecol[xw * le];
    t.B = Bp[xw * 8];
    t.b = bcol[x * 3 * S];
    t.lg = (dir < 0) ? gcol[x * 2 * S] : 0.0;
    return t;
  };
  double ch = 0.0, cl = 0.0;                                   // the sum over the tiles before this one
  k_in = k_out = -1;
  keep = ed_pm_nan();
  BoundsTile cur = load(0);
  for (int base = 0;; base += kWave) {
    const bool ahead = base > 0;
    BoundsTile nxt;
    if (ahead) nxt = load(base + kWave);
    const int k = base + lane;
    const bool valid = k <= kmax;
    double x = (valid && k > 0) ? cur.B + cur.e : 0.0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const double o = __shfl_up(x, d, kWave);
      x = (lane >= d) ? x + o : x;
    }
    const double head = (dir < 0) ? ((cur.lg == -HUGE_VAL ? cur.lg : cur.lg - cur.b) + head_a) : cur.b - head_a;
    const double G = (k == 0) ? 0.0 : head + ((ch + x) + cl);
    const unsigned long long f_in = ~__ballot(valid && G >= thi), f_out = ~__ballot(valid && G >= tlo);
    const bool last = base + kWave > kmax;
    if (k_in < 0 && (f_in || last)) k_in = f_in ? base + __ffsll((long long)f_in) - 2 : kmax;
    if (k_out < 0 && (f_out || last)) k_out = f_out ? base + __ffsll((long long)f_out) - 2 : kmax;
    if (kneed >= base && kneed < base + kWave) keep = __shfl(G, kneed - base, kWave);
    if (k_in >= 0 && k_out >= 0 && kneed < base + kWave) break;
    const double tot = __shfl(x, kWave - 1, kWave);
    if (tot - tot == 0.0 && ch - ch == 0.0) dd_add(ch, cl, tot);
    else { ch += tot; cl = 0.0; }                              // -inf (an impossible exon inside the row) stays -inf
    cur = ahead ? nxt : load(base + kWave);
  }
}

// One wavefront per call row (blockDim.x = kWave, blockIdx.x = row)
__global__ void __launch_bounds__(kWave)
k_call_bounds(const ed_call* __restrict__ calls, int64_t ncalls, const double* __restrict__ loglik, int64_t le, int64_t lst, int64_t ls,
              const double* __restrict__ lt4, const int32_t* __restrict__ chrom_off, int64_t S, const double* __restrict__ beta,
              const double* __restrict__ logpost, double thi, double tlo, ed_call_bounds* __restrict__ out)
{
  const int64_t r = blockIdx.x;
  if (r >= ncalls) return;
  const int lane = threadIdx.x;
  const ed_call c = calls[r];
  ed_call_bounds o;
  o.anchor_exon = o.start_lo = o.start_hi = c.start_exon;
  o.end_lo = o.end_hi = c.end_exon;
  o.flags = 1;
  o.log_anchor = o.log_keep_start = o.log_keep_end = ed_pm_nan();
  const int t = c.type;
  int ai = 0x7fffffff;
  double av = -HUGE_VAL;
  const int64_t s = c.sample;
  const double* __restrict__ gcol = logpost + (t == 2 ? 1 : 0) * S + s;           // exon x: gcol[x * 2 * S]
  if (t == 1 || t == 2) {
    // the anchor: every lane keeps the best of its exons (visited in rising order), then a butterfly over the lanes
#pragma unroll 4
    for (int64_t base = c.start_exon; base <= c.end_exon; base += kWave) {
      const int64_t xr = base + lane;
      const int64_t x = xr <= c.end_exon ? xr : (int64_t)c.end_exon;
      const double v = gcol[x * 2 * S];
      if (xr <= c.end_exon && v > av) { av = v; ai = (int)x; }
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) bounds_argmax(av, ai, __shfl_xor(av, d, kWave), __shfl_xor(ai, d, kWave));
  }
  if (ai == 0x7fffffff || av - av != 0.0) {                                      // another type, or no exon of the row has a finite log gamma(T)
    if (lane == 0) out[r] = o;
    return;
  }
  const int64_t a = ai;
  const int lo = chrom_off[c.chrom], hi = chrom_off[c.chrom + 1];
  const double* __restrict__ ecol = loglik + (t == 1 ? 0 : 2) * lst + s * ls;     // exon x: ecol[x * le]
  const double* __restrict__ Bp = lt4 + ((int64_t)c.chrom * 4 + 1) * 2;           // gap of exon x: x + chrom; lane 1's first entry is B
  const double* __restrict__ bcol = beta + (int64_t)t * S + s;                    // exon x: bcol[x * 3 * S]
  const double ba = bcol[a * 3 * S];
  int kl_in, kl_out, kr_in, kr_out;
  double keep_l, keep_r;
  bounds_walk<-1>(lane, a, (int)(a - lo), (int)(a - c.start_exon), ecol, le, Bp, bcol, gcol, S, ba - av, thi, tlo, kl_in, kl_out, keep_l);
  bounds_walk<1>(lane, a, (int)(hi - 1 - a), (int)(c.end_exon - a), ecol, le, Bp, bcol, gcol, S, ba, thi, tlo, kr_in, kr_out, keep_r);
  o.anchor_exon = ai;
  o.start_lo = ai - kl_out;
  o.start_hi = ai - kl_in;
  o.end_lo = ai + kr_in;
  o.end_hi = ai + kr_out;
  o.flags = 0;
  o.log_anchor = av;
  o.log_keep_start = keep_l;
  o.log_keep_end = keep_r;
  if (lane == 0) out[r] = o;
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// the two thresholds of a level, made here: log(tail) and log1p(-tail), tail = (1 - level) / 2
static bool bounds_thresholds(double level, double& thi, double& tlo)
{
  if (!(level > 0.0 && level < 1.0)) return false;             // (a NaN fails both)
  const double tail = (1.0 - level) / 2.0;
  tlo = std::log(tail);
  thi = std::log1p(-tail);
  return true;
}

static int bounds_launch(const ed_plan* p, const ed_call* d_calls, int64_t n, const double* d_loglik, int64_t S, const double* d_beta,
                         const double* d_logpost, double thi, double tlo, ed_call_bounds* d_out, hipStream_t st)
{
  hipLaunchKernelGGL(k_call_bounds, dim3((unsigned)n), dim3(kWave), 0, st, d_calls, n, d_loglik, 3 * S, S, (int64_t)1,
                     (const double*)p->d_lt3.get(), (const int32_t*)p->d_chrom_off.get(), S, d_beta, d_logpost, thi, tlo, d_out);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}

ED_EXPORT int ed_plan_call_bounds(const ed_plan* p, const ed_call* calls, int64_t n_calls, const double* d_loglik, int64_t n_samples,
                                  const double* d_work, const double* d_logpost, double level, ed_call_bounds* out, void* stream)
try {
  if (!p || n_calls < 0 || n_calls > 0x7fffffff || n_samples <= 0 || (n_calls > 0 && (!calls || !out || !d_loglik || !d_work || !d_logpost)))
    return ed_fail(ED_ERR_INVALID, "ed_plan_call_bounds: bad arguments");
  double thi, tlo;
  if (!bounds_thresholds(level, thi, tlo)) return ed_fail(ED_ERR_INVALID, "ed_plan_call_bounds: level must lie in (0, 1), got %g", level);
  if (int rc = check_call_rows("ed_plan_call_bounds", p, calls, n_calls, n_samples)) return rc;
  if (n_calls == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  DevBuf<ed_call> dc;
  DevBuf<ed_call_bounds> dout;
  if (dc.alloc((size_t)n_calls * sizeof(ed_call)) != hipSuccess || dout.alloc((size_t)n_calls * sizeof(ed_call_bounds)) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_plan_call_bounds: cannot allocate %lld rows", (long long)n_calls);
  HIP_TRY(hipMemcpyAsync(dc.get(), calls, (size_t)n_calls * sizeof(ed_call), hipMemcpyHostToDevice, st));
  if (int rc = bounds_launch(p, dc.get(), n_calls, d_loglik, n_samples, d_work, d_logpost, thi, tlo, dout.get(), st)) return rc;
  return ed_d2h(out, dout.get(), (size_t)n_calls * sizeof(ed_call_bounds), st);
}
ED_CATCH("ed_plan_call_bounds")

// The bounds of the last run's call table, behind the posterior's passes on the batch's stream (ensure_post): a request launches
// k_call_bounds alone once the passes are there, whatever its level.
ED_EXPORT int ed_batch_copy_call_bounds(ed_batch* b, double level, ed_call_bounds* host_out, int64_t cap)
try {
  double thi, tlo;
  if (!bounds_thresholds(level, thi, tlo)) return ed_fail(ED_ERR_INVALID, "ed_batch_copy_call_bounds: level must lie in (0, 1), got %g", level);
  int64_t n = 0;
  if (int rc = ed_batch_n_calls(b, &n)) return rc;   // (grows the table if the run needed more records)
  const int64_t k = std::min(n, cap);
  if (k <= 0) return ED_OK;
  if (!host_out) return ed_fail(ED_ERR_INVALID, "NULL output");
  if (int rc = ensure_post(b)) return rc;
  if (int rc = grow_records(b->req.d_cbounds, k, "call bounds")) return rc;
  EventSet<2>& ev = b->req.bounds_ev;
  const bool timed = b->timing;
  if (timed) { HIP_TRY(ev.ready()); HIP_TRY(ev.record(0, b->stream)); }
  if (int rc = bounds_launch(b->plan, b->d_calls.get(), k, b->d_loglik.get(), b->S, b->req.post.d_beta.get(), b->req.post.d_logpost.get(), thi, tlo,
                             b->req.d_cbounds.get(), b->stream))
    return rc;
  if (timed) HIP_TRY(ev.record(1, b->stream));
  ev.live = timed;
  return ed_d2h(host_out, b->req.d_cbounds, (size_t)k * sizeof(ed_call_bounds), b->stream);
}
ED_CATCH("ed_batch_copy_call_bounds")

// with ed_batch_enable_timing: the time of k_call_bounds of the last ed_batch_copy_call_bounds since the run's posterior was made, from
// events on its stream; 0 if not timed.  Synchronises that stream.
ED_EXPORT int ed_batch_call_bounds_ms(ed_batch* b, float* ms)
try {
  if (!b || !ms) return ed_fail(ED_ERR_INVALID, "NULL argument");
  return request_ms(b, b->req.bounds_ev, 0, 1, ms);
}
ED_CATCH("ed_batch_call_bounds_ms")
