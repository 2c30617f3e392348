// The score of the HMM's two transition parameters: d logZ / d t and d logZ / d L of every (sample, chromosome) chain (DESIGN.md 4.19).
//
// The model and its log-evidence are edpost.inc's.  By Fisher's identity the gradient of logZ is the posterior expectation of the
// gradient of the path's log-probability; the emissions do not depend on (t, L), so for theta in {t, L}
//   d logZ / d theta = sum_{i=1..m} sum_{k,j} xi_i(k->j) d lt_i[k->j] + sum_k gamma_m(k) d lt_{m+1}[k->0]
//   xi_i(k->j) = exp(alpha_{i-1}(k) + lt_i[k->j] + e_i(j) + beta_i(j) - logZ) = gamma_i(j) w_i(k | j)
// where w_i(. | j) are the softmax weights of the three operands of alpha_i(j)'s log-sum-exp: the forward step already forms their
// numerators and their sum.  The step then costs one exponential (gamma) and one reciprocal more than k_fb_forward's.
//
// k_fb_score is k_fb_forward's sibling: the same geometry (a quad per chain, lane j owns state j, lane 3 shadows state 0, 16 chains per
// wave, the batch's job tables), the same register ring (four steps deep: kScoreDepth) with its two-phase loop and clamped re-loads,
// ed_plog's table in LDS.  Next to the row of log-transitions it reads the row of their derivatives (ed_plan::d_dlt, ed_hmm_score.hpp: per gap and quad lane the four
// doubles (d/dt l.x, d/dt l.y, d/dL l.x, d/dL l.y)); lane j accumulates the terms of the transitions INTO state j, in exon order.  After
// the chain gamma_m(j) times the derivative of the closing step is added, and lanes 0, 1, 2 are summed in that order.
// One operation order per chain, no atomics, nothing shared between chains.  A chain whose logZ is not finite gets NaN.

namespace {

// The ring is edpost.inc's, four steps deep instead of kPostRing's eight -- emissions, beta, the rows of log-transitions and the rows of
// their derivatives alike.  Eight steps (each unrolled step holds the numerators of its weights until its sums are done) take 256 VGPRs and
// 56 to 88 AGPRs: no scratch, but one wave per SIMD, and a batch of 1 024 samples x 24 jobs is 1 536 waves on 1 024 SIMDs.  Four take 218
// VGPRs: two waves per SIMD, every wave of such a batch resident at once.  A step lasts about a microsecond, so four steps ahead is still
// several memory latencies.  Measured on that batch the two depths take the same time (23.2 and 23.0 ms: the pass lasts as long as its
// longest chain); the shallower ring is kept for the second wave per SIMD, which a wider batch fills.
constexpr int kScoreDepth = 4;

// lse3 (edpost.inc) that also hands out the softmax weights' numerators and the reciprocal of their sum.  `ok` is lse3's `sum >= 1`:
// false for a state no path reaches (all operands -inf), whose transitions carry no weight.
struct Lse3W {
  double v, e0, e1, e2, rs;
  bool ok;
};
__device__ __forceinline__ Lse3W lse3_w(double a, double b, double c, const double* logt)
{
  Lse3W o;
  const double m = __builtin_fmax(__builtin_fmax(a, b), c);
  o.e0 = ed_pexp(a - m); o.e1 = ed_pexp(b - m); o.e2 = ed_pexp(c - m);
  const double sum = (o.e0 + o.e1) + o.e2;
  const double r = m + ed_plog_core_t(sum, 0, logt);
  o.ok = sum >= 1.0;
  o.v = o.ok ? r : ((a + b) + c);
  // 1 / sum, sum in [1, 3] (or the value is not used): the hardware's estimate and two Newton steps, no scaling or special cases to serve
  double q = __builtin_amdgcn_rcp(sum);
  q = __builtin_fma(__builtin_fma(-sum, q, 1.0), q, q);
  o.rs = __builtin_fma(__builtin_fma(-sum, q, 1.0), q, q);
  return o;
}

// score [C][2][S]: row 0 d logZ / d t, row 1 d logZ / d L (zeroed by the host: an empty chromosome keeps 0); reads beta and logev as
// k_fb_backward left them.  dc0 = d c0 / d t, dc1 = d c1 / d t.
__global__ void __launch_bounds__(kWave)
k_fb_score(const double* __restrict__ loglik, int64_t le, int64_t lst, int64_t ls, const double* __restrict__ lt4,
           const double* __restrict__ dlt, double c0, double c1, double dc0, double dc1, const int32_t* __restrict__ chrom_off, int64_t S,
           const int32_t* __restrict__ job_off, const int32_t* __restrict__ job_chrom, const double* __restrict__ beta,
           const double* __restrict__ logev, double* __restrict__ score)
{
  const int lane = threadIdx.x;
  const int j = lane & 3;
  const int64_t s_raw = (int64_t)blockIdx.x * kVitChains + (lane >> 2);
  const bool live = s_raw < S;
  const int64_t s = live ? s_raw : S - 1;   // idle quads shadow the last sample (loads stay in bounds, no stores)
  const bool st0 = (j == 0 || j == 3);
  const int hs = st0 ? 0 : j;
  const int col = (j == 1) ? 0 : ((j == 2) ? 2 : 1);
  const double t0 = st0 ? c0 : c1;
  const double dt0 = st0 ? dc0 : dc1;       // d/dt of the entry out of normal into this lane's state (its d/dL is 0)
  const int job = (int)blockIdx.y;
  __shared__ double logt[ED_PM_LOGT_N * 3];
  post_park_logt(logt, lane);
  // (no job tables lent -- ed_plan_transition_score: a workgroup per chromosome, in index order)
  for (int jc = job_off ? job_off[job] : job, je = job_off ? job_off[job + 1] : job + 1; jc < je; ++jc) {
    const int c = job_off ? job_chrom[jc] : jc;
    const int64_t lo = chrom_off[c];
    const int m = chrom_off[c + 1] - chrom_off[c];
    if (m <= 0) continue;
    const double* __restrict__ eb = loglik + lo * le + col * lst + s * ls;
    const double2* __restrict__ lp = reinterpret_cast<const double2*>(lt4) + (lo + c) * 4 + j;          // gap g: lp[g * 4]
    const double4* __restrict__ dp = reinterpret_cast<const double4*>(dlt) + (lo + c) * 4 + j;          // gap g: dp[g * 4]
    const double* __restrict__ bb = beta + (lo * 3 + hs) * S + s;
    const int64_t bstride = 3 * S;
    const double lz = logev[(int64_t)c * S + s];
    double al = st0 ? 0.0 : -HUGE_VAL;
    double gm = 0.0;                         // gamma of the last step taken
    double acc_t = 0.0, acc_l = 0.0;
    auto at = [&](int q) { return q < m ? q : m - 1; };
    double er[kScoreDepth], br[kScoreDepth];
    double2 lr[kScoreDepth];
    double4 dr[kScoreDepth];
#pragma unroll
    for (int k = 0; k < kScoreDepth; ++k) {
      const int i = at(k);
      er[k] = eb[(int64_t)i * le];
      lr[k] = lp[(int64_t)i * 4];
      dr[k] = dp[(int64_t)i * 4];
      br[k] = bb[(int64_t)i * bstride];
    }
    auto step = [&](int k) {
      const double2 l = lr[k];
      const double4 d = dr[k];
      const double a0 = quad_bcast<0>(al), a1 = quad_bcast<1>(al), a2 = quad_bcast<2>(al);
      const Lse3W w = lse3_w(a0 + t0, a1 + l.x, a2 + l.y, logt);
      al = er[k] + w.v;
      gm = ed_pexp((al + br[k]) - lz);       // gamma_i(j)
      const double g = gm * w.rs;
      const double ut = (w.e0 * dt0 + w.e1 * d.x) + w.e2 * d.y;
      const double ul = w.e1 * d.z + w.e2 * d.w;
      acc_t += w.ok ? g * ut : 0.0;
      acc_l += w.ok ? g * ul : 0.0;
    };
    int base = 0;
    for (; base + 2 * kScoreDepth <= m; base += kScoreDepth) {   // whole rings whose re-loads stay inside the chain: one straight block
#pragma unroll
      for (int k = 0; k < kScoreDepth; ++k) {
        const int i = base + k;
        step(k);
        er[k] = eb[(int64_t)(i + kScoreDepth) * le];
        lr[k] = lp[(int64_t)(i + kScoreDepth) * 4];
        dr[k] = dp[(int64_t)(i + kScoreDepth) * 4];
        br[k] = bb[(int64_t)(i + kScoreDepth) * bstride];
      }
    }
    for (; base < m; base += kScoreDepth) {                    // the last one or two rings: guarded steps, clamped re-loads
#pragma unroll
      for (int k = 0; k < kScoreDepth; ++k) {
        const int i = base + k;
        if (i < m) {
          step(k);
          const int in = at(i + kScoreDepth);
          er[k] = eb[(int64_t)in * le];
          lr[k] = lp[(int64_t)in * 4];
          dr[k] = dp[(int64_t)in * 4];
          br[k] = bb[(int64_t)in * bstride];
        }
      }
    }
    // the closing step: gamma_m(j) d lt_{m+1}[j->0]; out of normal that is c0, out of a CNV state the closing gap's A (lane 0's first entry)
    {
      const double4 d = dp[(int64_t)m * 4];
      const double dAt = quad_bcast<0>(d.x), dAl = quad_bcast<0>(d.z);
      acc_t += gm * (st0 ? dc0 : dAt);
      acc_l += gm * (st0 ? 0.0 : dAl);
    }
    const double sum_t = (quad_bcast<0>(acc_t) + quad_bcast<1>(acc_t)) + quad_bcast<2>(acc_t);   // lane 3 shadows state 0: not counted
    const double sum_l = (quad_bcast<0>(acc_l) + quad_bcast<1>(acc_l)) + quad_bcast<2>(acc_l);
    const bool fin = (lz - lz) == 0.0;       // logZ finite
    if (live && j < 2) score[((int64_t)c * 2 + j) * S + s] = fin ? (j == 0 ? sum_t : sum_l) : ed_pm_nan();
  }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// The plan's table of derivatives, built from the padded positions ed_plan_create kept and uploaded on the first request: once, under
// the plan's lock.  (A synchronous copy: the table is complete on the device when this returns, whatever stream reads it.)
static int ensure_score_table(const ed_plan* p)
{
  std::lock_guard<std::mutex> lock(p->score_mu);
  if (p->d_dlt) return ED_OK;
  const size_t n = (size_t)std::max<int64_t>(p->E + p->C, 1) * edscore::kRow;
  std::vector<double> tab(n, 0.0);
  edscore::fill_table(p->tprob, p->L, p->C, p->chrom_off.data(), p->pad_pos.data(), tab.data());
  DevBuf<double> d;
  if (d.alloc(n * 8) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "transition score: cannot allocate the table of derivatives (%lld gaps)", (long long)(p->E + p->C));
  HIP_TRY(hipMemcpy(d.get(), tab.data(), n * 8, hipMemcpyHostToDevice));
  p->d_dlt = std::move(d);
  ++p->score_tables;
  return ED_OK;
}

// the score pass on `st`, behind the backward pass that left d_beta and d_logev
static int score_launch(const ed_plan* p, const double* d_loglik, int64_t S, const double* d_beta, const double* d_logev, double* d_score,
                        const int32_t* d_job_off, const int32_t* d_job_chrom, int32_t n_jobs, hipStream_t st)
{
  if (p->C <= 0) return ED_OK;
  HIP_TRY(hipMemsetAsync(d_score, 0, (size_t)p->C * 2 * S * 8, st));     // an empty chromosome is in no job: its score is 0
  if (n_jobs <= 0) return ED_OK;
  const dim3 grid((unsigned)((S + kVitChains - 1) / kVitChains), (unsigned)n_jobs);
  hipLaunchKernelGGL(k_fb_score, grid, dim3(kWave), 0, st, d_loglik, 3 * S, S, (int64_t)1, (const double*)p->d_lt3.get(),
                     (const double*)p->d_dlt.get(), p->c0, p->c1, edscore::dc0_dt(p->tprob), edscore::dc1_dt(p->tprob), p->d_chrom_off.get(), S,
                     d_job_off, d_job_chrom, d_beta, d_logev, d_score);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}

ED_EXPORT int ed_plan_transition_score(const ed_plan* p, const double* d_loglik, int64_t n_samples, double* d_work, double* d_log_evidence,
                                       double* d_score, void* stream)
try {
  if (!p || n_samples <= 0 || n_samples > 32768 || !d_log_evidence || !d_score || (p->E > 0 && (!d_loglik || !d_work)))
    return ed_fail(ED_ERR_INVALID, "ed_plan_transition_score: bad arguments (1 <= n_samples <= 32768, no NULL array)");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if (p->C > 65535) return ed_fail(ED_ERR_INVALID, "ed_plan_transition_score: more than 65535 chromosomes");
  if (p->C <= 0) return ED_OK;
  if (int rc = ensure_score_table(p)) return rc;
  const int64_t S = n_samples;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_log_evidence, 0, (size_t)p->C * S * 8, st));
  const dim3 grid((unsigned)((S + kVitChains - 1) / kVitChains), (unsigned)p->C);
  hipLaunchKernelGGL(k_fb_backward, grid, dim3(kWave), 0, st, d_loglik, 3 * S, S, (int64_t)1, (const double*)p->d_lt3.get(), p->c0, p->c1,
                     p->d_chrom_off.get(), S, (const int32_t*)nullptr, (const int32_t*)nullptr, d_work, d_log_evidence);
  HIP_TRY(hipGetLastError());
  return score_launch(p, d_loglik, S, d_work, d_log_evidence, d_score, nullptr, nullptr, p->C, st);
}
ED_CATCH("ed_plan_transition_score")

// The score of the batch's last run, made when somebody asks, as the posterior is (ensure_post): behind its passes on the same stream,
// reading their beta and logZ; with an asynchronous tail done_ev is moved behind the score pass as well.
static int ensure_score(ed_batch* b)
{
  if (b->req.score_valid) return ED_OK;
  if (int rc = ensure_post(b)) return rc;
  const ed_plan* p = b->plan;
  if (int rc = ensure_score_table(p)) return rc;
  if (!b->req.d_score) {
    if (b->req.d_score.alloc((size_t)std::max<int64_t>(p->C, 1) * 2 * b->S * 8) != hipSuccess)
      return ed_fail(ED_ERR_NOMEM, "transition score: cannot allocate %lld x 2 x %lld values", (long long)p->C, (long long)b->S);
  }
  const bool timed = b->timing && p->C > 0 && b->n_jobs > 0;
  EventSet<2>& ev = b->req.score_ev;
  if (timed) { HIP_TRY(ev.ready()); HIP_TRY(ev.record(0, b->stream)); }
  if (int rc = score_launch(p, b->d_loglik, b->S, b->req.post.d_beta, b->req.post.d_logev, b->req.d_score, b->d_job_off, b->d_job_chrom, b->n_jobs,
                            b->stream))
    return rc;
  if (timed) HIP_TRY(ev.record(1, b->stream));
  ev.live = timed;
  if (b->last.async && b->done_ev) HIP_TRY(hipEventRecord(b->done_ev, b->stream));
  ++b->req.score_passes;
  b->req.score_valid = true;
  return ED_OK;
}

ED_EXPORT int ed_batch_copy_transition_score(ed_batch* b, double* host_score)
try {
  if (int rc = batch_ready(b)) return rc;
  if (!host_score) return ed_fail(ED_ERR_INVALID, "NULL output");
  if (int rc = ensure_score(b)) return rc;
  return ed_d2h(host_score, b->req.d_score, (size_t)b->plan->C * 2 * b->S * 8, b->stream);
}
ED_CATCH("ed_batch_copy_transition_score")

// how many times the score pass has been enqueued on this batch since it was created (a request after the first launches nothing)
ED_EXPORT int64_t ed_batch_n_score_passes(const ed_batch* b) { return b ? b->req.score_passes : 0; }

// how many times this plan has built and uploaded its table of derivatives (0 before the first request, 1 ever after)
ED_EXPORT int64_t ed_plan_n_score_tables(const ed_plan* p) { return p ? p->score_tables : 0; }

// with ed_batch_enable_timing: the time of k_fb_score of the last run's score request, from events on its stream; 0 if not timed.
// Synchronises that stream.
ED_EXPORT int ed_batch_transition_score_ms(ed_batch* b, float* ms)
try {
  if (!b || !ms) return ed_fail(ED_ERR_INVALID, "NULL argument");
  return request_ms(b, b->req.score_ev, 0, 1, ms);
}
ED_CATCH("ed_batch_transition_score_ms")
