// Forward-backward on the three-state HMM of k_viterbi: exon posteriors, chain log-evidence, per-call confidence (DESIGN.md 4.18).
//
// The model is k_viterbi's (the comment block above it in edcore.hip): HMM states 0 normal, 1 deletion, 2 duplication; state j reads
// likelihood column {1, 0, 2}[j]; a chain (one sample x one chromosome) of m exons starts from alpha_0 = (0, -inf, -inf) and ends
// with the dummy observation whose state is forced to 0 (src/hmm.cpp:96), so
//   alpha_i(j)  = e_i(j) + LSE_k(alpha_{i-1}(k) + lt_i[k->j])                      i = 1 .. m
//   beta_m(k)   = lt_{m+1}[k->0]
//   beta_{i-1}(k) = LSE_j(lt_i[k->j] + (e_i(j) + beta_i(j)))                       i = m .. 1
//   logZ        = beta_0(0)   ( = LSE_k(alpha_m(k) + lt_{m+1}[k->0]) )
//   log gamma_i(j) = (alpha_i(j) + beta_i(j)) - logZ
// lt_i are the plan's values (ed_plan::d_lt3): from normal (c0, c1, c1); from state 1 / 2 the per-gap triple (A into normal, B stay,
// C switch) the table holds per quad lane as (A, A), (B, C), (C, B); gap of exon i (0-based) of chromosome c: lo + c + i, the closing
// step at lo + c + m.
//
// Geometry: k_viterbi's.  A quad of lanes per chain (lane j owns state j, the 4th lane shadows state 0), the other states' values two
// DPP quad-broadcasts away, 16 chains per wave, idle quads shadow the last sample and store nothing, a workgroup walks the chromosomes
// of its job.  Emissions, rows of log-transitions and (forward) beta sit in a register ring kPostRing steps ahead of their use.  Whole
// rings whose re-loads stay inside the chain run as one straight block (the re-loads stay in flight across its steps); the last one or
// two rings take guarded steps whose re-load index is clamped to the chain, so no load leaves the chromosome.  A step is dominated by
// the three exponentials and the logarithm of its log-sum-exp -- an order of magnitude more arithmetic than a Viterbi step -- which is why
// the transition rows are read from the table directly (every quad the same 64 bytes: one L1 line per step) and not parked in LDS.  What
// IS parked in LDS is ed_plog's table (3 KB): see lse3.
// One operation order per chain, no atomics, nothing shared between chains: a sample's values do not depend on its batch-mates.
//
// The backward pass runs first and leaves logZ = beta_0(0); the forward pass needs it as the normaliser from its first exon on.

namespace {

constexpr int kPostRing = 8;

// log(exp(a) + exp(b) + exp(c)) = m + ed_plog(sum), m the largest operand (maxNum: a NaN operand loses), sum in [1, 3] because the
// largest term is ed_pexp(0) = 1 exactly.  ed_plog's table is read from the copy the kernel parked in LDS (`logt`; ed_plog_core_t is
// ed_plog's arithmetic for a positive normal argument): a table load from memory would have to be waited for with vmcnt(0), and that wait
// also ends the flight of every ring re-load issued before it -- the step would pay a full memory latency.  Anything else -- a NaN operand,
// all operands -inf (the differences are NaN) -- makes `sum >= 1` false, and the plain sum of the operands is the answer: NaN, or -inf.
__device__ __forceinline__ double lse3(double a, double b, double c, const double* logt)
{
  const double m = __builtin_fmax(__builtin_fmax(a, b), c);
  const double sum = (ed_pexp(a - m) + ed_pexp(b - m)) + ed_pexp(c - m);
  const double r = m + ed_plog_core_t(sum, 0, logt);
  return (sum >= 1.0) ? r : ((a + b) + c);
}

// the wave's copy of ed_plog's table (ED_PM_LOGT_N rows of 3 doubles)
__device__ __forceinline__ void post_park_logt(double* logt, int lane)
{
  const double T[ED_PM_LOGT_N][3] = ED_PM_LOGT_ROWS;
  for (int i = lane; i < ED_PM_LOGT_N * 3; i += kWave) logt[i] = (&T[0][0])[i];
  __syncthreads();
}

// beta [E][3][S] in HMM state order (row 0 normal, 1 deletion, 2 duplication); logev [C][S] (zeroed by the host: an empty chromosome keeps 0)
__global__ void __launch_bounds__(kWave)
k_fb_backward(const double* __restrict__ loglik, int64_t le, int64_t lst, int64_t ls,   // likelihood element (e, st, s) at e * le + st * lst + s * ls
              const double* __restrict__ lt4, double c0, double c1, const int32_t* __restrict__ chrom_off, int64_t S,
              const int32_t* __restrict__ job_off, const int32_t* __restrict__ job_chrom, double* __restrict__ beta,
              double* __restrict__ logev)
{
  const int lane = threadIdx.x;
  const int j = lane & 3;
  const int64_t s_raw = (int64_t)blockIdx.x * kVitChains + (lane >> 2);
  const bool live = s_raw < S;
  const int64_t s = live ? s_raw : S - 1;   // idle quads shadow the last sample (loads stay in bounds, no stores)
  const bool st0 = (j == 0 || j == 3);
  const int hs = st0 ? 0 : j;
  const int col = (j == 1) ? 0 : ((j == 2) ? 2 : 1);
  const bool wr = live && j < 3;
  const int job = (int)blockIdx.y;
  __shared__ double logt[ED_PM_LOGT_N * 3];
  post_park_logt(logt, lane);
  // (no job tables lent -- ed_plan_posterior without a batch: a workgroup per chromosome, in index order)
  for (int jc = job_off ? job_off[job] : job, je = job_off ? job_off[job + 1] : job + 1; jc < je; ++jc) {
    const int c = job_off ? job_chrom[jc] : jc;
    const int64_t lo = chrom_off[c];
    const int m = chrom_off[c + 1] - chrom_off[c];
    if (m <= 0) continue;
    const double* __restrict__ eb = loglik + lo * le + col * lst + s * ls;                              // exon i: eb[i * le]
    const double2* __restrict__ lp = reinterpret_cast<const double2*>(lt4) + (lo + c) * 4 + j;           // gap g: lp[g * 4]
    double* __restrict__ bb = beta + (lo * 3 + hs) * S + s;                                             // exon i: bb[i * 3 * S]
    const int64_t bstride = 3 * S;
    double bt;
    {
      const double2 l = lp[(int64_t)m * 4];
      const double A = quad_bcast<0>(l.x);
      bt = st0 ? c0 : A;                       // beta_m(k) = lt_{m+1}[k->0]
    }
    if (wr) bb[(int64_t)(m - 1) * bstride] = bt;
    // step q handles exon i = m - 1 - q
    auto at = [&](int q) { const int i = m - 1 - q; return i > 0 ? i : 0; };
    double er[kPostRing];
    double2 lr[kPostRing];
#pragma unroll
    for (int k = 0; k < kPostRing; ++k) {
      const int i = at(k);
      er[k] = eb[(int64_t)i * le];
      lr[k] = lp[(int64_t)i * 4];
    }
    auto step = [&](int k, int i) {
      const double g = er[k] + bt;
      const double2 l = lr[k];
      const double g0 = quad_bcast<0>(g), g1 = quad_bcast<1>(g), g2 = quad_bcast<2>(g);
      const double A = quad_bcast<0>(l.x);
      const double u0 = st0 ? c0 : A, u1 = st0 ? c1 : l.x, u2 = st0 ? c1 : l.y;
      bt = lse3(u0 + g0, u1 + g1, u2 + g2, logt);         // beta_{i-1}(k)
    };
    int base = 0;
    // whole rings whose re-loads stay inside the chain (exon i - kPostRing >= 0) and whose stores all exist (i >= 1): one straight block,
    // so that the re-loads stay in flight across the steps
    for (; base + 2 * kPostRing <= m; base += kPostRing) {
#pragma unroll
      for (int k = 0; k < kPostRing; ++k) {
        const int i = m - 1 - (base + k);
        step(k, i);
        if (wr) bb[(int64_t)(i - 1) * bstride] = bt;
        er[k] = eb[(int64_t)(i - kPostRing) * le];
        lr[k] = lp[(int64_t)(i - kPostRing) * 4];
      }
    }
    for (; base < m; base += kPostRing) {    // the last one or two rings: guarded steps, clamped re-loads
#pragma unroll
      for (int k = 0; k < kPostRing; ++k) {
        const int q = base + k;
        if (q < m) {
          const int i = m - 1 - q;
          step(k, i);
          if (i > 0) {
            if (wr) bb[(int64_t)(i - 1) * bstride] = bt;
          } else if (live && j == 0) {
            logev[(int64_t)c * S + s] = bt;                // beta_0(0) = logZ
          }
          const int in = at(q + kPostRing);
          er[k] = eb[(int64_t)in * le];
          lr[k] = lp[(int64_t)in * 4];
        }
      }
    }
  }
}

// logpost [E][2][S]: log gamma of deletion (row 0) and duplication (row 1); reads beta and logev as k_fb_backward left them
__global__ void __launch_bounds__(kWave)
k_fb_forward(const double* __restrict__ loglik, int64_t le, int64_t lst, int64_t ls, const double* __restrict__ lt4, double c0, double c1,
             const int32_t* __restrict__ chrom_off, int64_t S, const int32_t* __restrict__ job_off, const int32_t* __restrict__ job_chrom,
             const double* __restrict__ beta, const double* __restrict__ logev, double* __restrict__ logpost)
{
  const int lane = threadIdx.x;
  const int j = lane & 3;
  const int64_t s_raw = (int64_t)blockIdx.x * kVitChains + (lane >> 2);
  const bool live = s_raw < S;
  const int64_t s = live ? s_raw : S - 1;
  const bool st0 = (j == 0 || j == 3);
  const int hs = st0 ? 0 : j;
  const int col = (j == 1) ? 0 : ((j == 2) ? 2 : 1);
  const bool wr = live && (j == 1 || j == 2);
  const double t0 = st0 ? c0 : c1;
  const int job = (int)blockIdx.y;
  __shared__ double logt[ED_PM_LOGT_N * 3];
  post_park_logt(logt, lane);
  // (no job tables lent -- ed_plan_posterior without a batch: a workgroup per chromosome, in index order)
  for (int jc = job_off ? job_off[job] : job, je = job_off ? job_off[job + 1] : job + 1; jc < je; ++jc) {
    const int c = job_off ? job_chrom[jc] : jc;
    const int64_t lo = chrom_off[c];
    const int m = chrom_off[c + 1] - chrom_off[c];
    if (m <= 0) continue;
    const double* __restrict__ eb = loglik + lo * le + col * lst + s * ls;
    const double2* __restrict__ lp = reinterpret_cast<const double2*>(lt4) + (lo + c) * 4 + j;
    const double* __restrict__ bb = beta + (lo * 3 + hs) * S + s;
    const int64_t bstride = 3 * S;
    double* __restrict__ ob = logpost + (lo * 2 + (j == 2 ? 1 : 0)) * S + s;                            // exon i: ob[i * 2 * S]
    const int64_t ostride = 2 * S;
    const double lz = logev[(int64_t)c * S + s];
    double al = st0 ? 0.0 : -HUGE_VAL;
    auto at = [&](int q) { return q < m ? q : m - 1; };
    double er[kPostRing], br[kPostRing];
    double2 lr[kPostRing];
#pragma unroll
    for (int k = 0; k < kPostRing; ++k) {
      const int i = at(k);
      er[k] = eb[(int64_t)i * le];
      lr[k] = lp[(int64_t)i * 4];
      br[k] = bb[(int64_t)i * bstride];
    }
    auto step = [&](int k, int i) {
      const double2 l = lr[k];
      const double a0 = quad_bcast<0>(al), a1 = quad_bcast<1>(al), a2 = quad_bcast<2>(al);
      al = er[k] + lse3(a0 + t0, a1 + l.x, a2 + l.y, logt);
      const double lg = (al + br[k]) - lz;
      if (wr) ob[(int64_t)i * ostride] = lg;
    };
    int base = 0;
    for (; base + 2 * kPostRing <= m; base += kPostRing) {   // whole rings whose re-loads stay inside the chain: one straight block
#pragma unroll
      for (int k = 0; k < kPostRing; ++k) {
        const int i = base + k;
        step(k, i);
        er[k] = eb[(int64_t)(i + kPostRing) * le];
        lr[k] = lp[(int64_t)(i + kPostRing) * 4];
        br[k] = bb[(int64_t)(i + kPostRing) * bstride];
      }
    }
    for (; base < m; base += kPostRing) {                    // the last one or two rings: guarded steps, clamped re-loads
#pragma unroll
      for (int k = 0; k < kPostRing; ++k) {
        const int i = base + k;
        if (i < m) {
          step(k, i);
          const int in = at(i + kPostRing);
          er[k] = eb[(int64_t)in * le];
          lr[k] = lp[(int64_t)in * 4];
          br[k] = bb[(int64_t)in * bstride];
        }
      }
    }
  }
}

// One thread per call row, as k_call_info.  A call of type t over exons a..b of its chain:
//   post_mean, post_min   of exp(log gamma_i(t)), i = a..b
//   log_p_all = log gamma_a(t) + sum_{i=a+1..b} (lt_i[t->t] + e_i(t)) + beta_b(t) - beta_a(t): every exon of the row in state t (the sum
//               carried as a double-double, rounded once)
//   log_evidence          of the row's chain
__global__ void k_call_post(const ed_call* __restrict__ calls, int64_t ncalls, const double* __restrict__ loglik, int64_t le, int64_t lst,
                            int64_t ls, const double* __restrict__ lt4, int64_t S, const double* __restrict__ beta,
                            const double* __restrict__ logpost, const double* __restrict__ logev, ed_call_post* __restrict__ out)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ncalls) return;
  const ed_call c = calls[r];
  ed_call_post o;
  if (c.type != 1 && c.type != 2) {
    o.post_mean = o.post_min = o.log_p_all = o.log_evidence = ed_pm_nan();
    out[r] = o;
    return;
  }
  const int64_t s = c.sample, a = c.start_exon, b = c.end_exon;
  const int t = c.type;
  const int col = (t == 1) ? 0 : 2;
  double sum = 0.0, mn = HUGE_VAL, sh = 0.0, sl = 0.0;
  for (int64_t e = a; e <= b; ++e) {
    const double p = ed_pexp(logpost[(e * 2 + (t - 1)) * S + s]);
    sum += p;
    mn = (p < mn || p != p) ? p : mn;
    if (e > a) {
      const double B = lt4[((e + c.chrom) * 4 + 1) * 2];      // gap of exon e: lo + chrom + (e - lo); lane 1's first entry is B
      dd_add(sh, sl, B + loglik[e * le + col * lst + s * ls]);
    }
  }
  o.post_mean = sum / (double)(b - a + 1);
  o.post_min = mn;
  o.log_p_all = ((logpost[(a * 2 + (t - 1)) * S + s] + (sh + sl)) + beta[(b * 3 + t) * S + s]) - beta[(a * 3 + t) * S + s];
  o.log_evidence = logev[(int64_t)c.chrom * S + s];
  out[r] = o;
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// the two passes on `st`; the job tables are the batch's (n_jobs of them), or NULL with n_jobs = the plan's chromosomes
static int post_launch(const ed_plan* p, const double* d_loglik, int64_t le, int64_t lst, int64_t ls, int64_t S, double* d_beta,
                       double* d_logpost, double* d_logev, const int32_t* d_job_off, const int32_t* d_job_chrom, int32_t n_jobs,
                       hipStream_t st, hipEvent_t between = nullptr)
{
  if (p->C <= 0) return ED_OK;
  HIP_TRY(hipMemsetAsync(d_logev, 0, (size_t)p->C * S * 8, st));     // an empty chromosome is in no job: its log-evidence is 0
  if (n_jobs <= 0) return ED_OK;
  const dim3 grid((unsigned)((S + kVitChains - 1) / kVitChains), (unsigned)n_jobs);
  hipLaunchKernelGGL(k_fb_backward, grid, dim3(kWave), 0, st, d_loglik, le, lst, ls, p->d_lt3.get(), p->c0, p->c1, p->d_chrom_off.get(), S,
                     d_job_off, d_job_chrom, d_beta, d_logev);
  HIP_TRY(hipGetLastError());
  if (between) HIP_TRY(hipEventRecord(between, st));
  hipLaunchKernelGGL(k_fb_forward, grid, dim3(kWave), 0, st, d_loglik, le, lst, ls, p->d_lt3.get(), p->c0, p->c1, p->d_chrom_off.get(), S,
                     d_job_off, d_job_chrom, (const double*)d_beta, (const double*)d_logev, d_logpost);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}

ED_EXPORT int ed_plan_posterior(const ed_plan* p, const double* d_loglik, int64_t n_samples, double* d_work, double* d_logpost,
                                double* d_log_evidence, void* stream)
try {
  if (!p || n_samples <= 0 || n_samples > 32768 || !d_log_evidence || (p->E > 0 && (!d_loglik || !d_work || !d_logpost)))
    return ed_fail(ED_ERR_INVALID, "ed_plan_posterior: bad arguments (1 <= n_samples <= 32768, no NULL array)");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if (p->C > 65535) return ed_fail(ED_ERR_INVALID, "ed_plan_posterior: more than 65535 chromosomes");
  return post_launch(p, d_loglik, 3 * n_samples, n_samples, 1, n_samples, d_work, d_logpost, d_log_evidence, nullptr, nullptr, p->C,
                     (hipStream_t)stream);
}
ED_CATCH("ed_plan_posterior")

ED_EXPORT int ed_plan_call_posterior(const ed_plan* p, const ed_call* calls, int64_t n_calls, const double* d_loglik, int64_t n_samples,
                                     const double* d_work, const double* d_logpost, const double* d_log_evidence, ed_call_post* out,
                                     void* stream)
try {
  if (!p || n_calls < 0 || n_samples <= 0 || (n_calls > 0 && (!calls || !out || !d_loglik || !d_work || !d_logpost || !d_log_evidence)))
    return ed_fail(ED_ERR_INVALID, "ed_plan_call_posterior: bad arguments");
  if (int rc = check_call_rows("ed_plan_call_posterior", p, calls, n_calls, n_samples)) return rc;
  if (n_calls == 0) return ED_OK;
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  DevBuf<ed_call> dc;
  DevBuf<ed_call_post> dout;
  if (dc.alloc((size_t)n_calls * sizeof(ed_call)) != hipSuccess || dout.alloc((size_t)n_calls * sizeof(ed_call_post)) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_plan_call_posterior: cannot allocate %lld rows", (long long)n_calls);
  HIP_TRY(hipMemcpyAsync(dc.get(), calls, (size_t)n_calls * sizeof(ed_call), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_call_post, dim3((unsigned)((n_calls + 127) / 128)), dim3(128), 0, st, (const ed_call*)dc.get(), n_calls, d_loglik,
                     3 * n_samples, n_samples, (int64_t)1, p->d_lt3.get(), n_samples, d_work, d_logpost, d_log_evidence, dout.get());
  HIP_TRY(hipGetLastError());
  return ed_d2h(out, dout.get(), (size_t)n_calls * sizeof(ed_call_post), st);
}
ED_CATCH("ed_plan_call_posterior")

// The posterior of the batch's last run, made when somebody asks (as ensure_path makes the byte path): on the stream the run's results
// become available on, behind the run; with an asynchronous tail done_ev is moved behind the passes, so that the batch's next run
// (which rewrites the likelihood matrix) waits for them as it does for the tail.  The buffers are there or they are not.
static int ensure_post(ed_batch* b)
{
  if (b->req.post_valid) return ED_OK;
  if (b->fused && !b->keep_loglik)
    return ed_fail(ED_ERR_STATE, "the posterior reads the likelihood matrix, which this fused batch does not keep (ed_batch_keep_loglik(batch, 1))");
  HIP_TRY(hipSetDevice(b->plan->device));
  if (int rc = ensure_loglik_rows(b)) return rc;      // emit mode 2: through the [E][3][S] form
  if (!b->d_loglik) return ed_fail(ED_ERR_STATE, "the posterior reads the likelihood matrix, which is not kept (ed_batch_keep_loglik)");
  const ed_plan* p = b->plan;
  const int64_t E = p->E, S = b->S, C = p->C;
  if (!b->req.post.made()) {
    PostSet t;
    if (t.d_beta.alloc((size_t)std::max<int64_t>(E, 1) * 3 * S * 8) != hipSuccess ||
        t.d_logpost.alloc((size_t)std::max<int64_t>(E, 1) * 2 * S * 8) != hipSuccess ||
        t.d_logev.alloc((size_t)std::max<int64_t>(C, 1) * S * 8) != hipSuccess)
      return ed_fail(ED_ERR_NOMEM, "posterior: cannot allocate 40 bytes per cell (E=%lld S=%lld)", (long long)E, (long long)S);
    b->req.post = std::move(t);
  }
  const bool timed = b->timing && p->C > 0 && b->n_jobs > 0;
  EventSet<3>& ev = b->req.post_ev;
  ev.drop(); b->req.cpost_ev.drop(); b->req.bounds_ev.drop();     // they time readers of the posterior that these passes replace
  if (timed) { HIP_TRY(ev.ready()); HIP_TRY(ev.record(0, b->stream)); }
  if (int rc = post_launch(p, b->d_loglik, 3 * S, S, 1, S, b->req.post.d_beta, b->req.post.d_logpost, b->req.post.d_logev, b->d_job_off, b->d_job_chrom,
                           b->n_jobs, b->stream, timed ? ev.ev[1].get() : nullptr))
    return rc;
  if (timed) HIP_TRY(ev.record(2, b->stream));
  ev.live = timed;
  if (b->last.async && b->done_ev) HIP_TRY(hipEventRecord(b->done_ev, b->stream));
  ++b->req.post_passes;
  b->req.post_valid = true;
  return ED_OK;
}

ED_EXPORT int ed_batch_copy_posterior(ed_batch* b, double* host_logpost)
try {
  if (int rc = batch_ready(b)) return rc;
  if (!host_logpost) return ed_fail(ED_ERR_INVALID, "NULL output");
  if (int rc = ensure_post(b)) return rc;
  return ed_d2h(host_logpost, b->req.post.d_logpost, (size_t)b->plan->E * 2 * b->S * 8, b->stream);
}
ED_CATCH("ed_batch_copy_posterior")

ED_EXPORT int ed_batch_copy_log_evidence(ed_batch* b, double* host_log_evidence)
try {
  if (int rc = batch_ready(b)) return rc;
  if (!host_log_evidence) return ed_fail(ED_ERR_INVALID, "NULL output");
  if (int rc = ensure_post(b)) return rc;
  return ed_d2h(host_log_evidence, b->req.post.d_logev, (size_t)b->plan->C * b->S * 8, b->stream);
}
ED_CATCH("ed_batch_copy_log_evidence")

// (the first call after a run enqueues the passes and waits for them: the pointer's reader is on a stream of its own)
ED_EXPORT const double* ed_batch_posterior(const ed_batch* b_)
{
  ed_batch* b = const_cast<ed_batch*>(b_);
  if (!b || !b->ran) { (void)ed_fail(ED_ERR_STATE, "ed_batch_posterior: no ed_batch_run has been issued on this batch"); return nullptr; }
  if (!b->req.post_valid) {
    if (ensure_post(b) != ED_OK) return nullptr;
    if (hipStreamSynchronize(b->stream) != hipSuccess) { (void)ed_fail(ED_ERR_HIP, "ed_batch_posterior: the run or the posterior passes failed"); return nullptr; }
  }
  return b->req.post.d_logpost;
}

ED_EXPORT int ed_batch_copy_call_posterior(ed_batch* b, ed_call_post* host_post, int64_t cap)
try {
  int64_t n = 0;
  if (int rc = ed_batch_n_calls(b, &n)) return rc;   // (grows the table if the run needed more records)
  const int64_t k = std::min(n, cap);
  if (k <= 0) return ED_OK;
  if (!host_post) return ed_fail(ED_ERR_INVALID, "NULL output");
  if (int rc = ensure_post(b)) return rc;
  if (int rc = grow_records(b->req.d_cpost, k, "call posterior")) return rc;
  EventSet<2>& ev = b->req.cpost_ev;
  const bool timed = b->timing && b->req.post_ev.live;
  if (timed) { HIP_TRY(ev.ready()); HIP_TRY(ev.record(0, b->stream)); }
  hipLaunchKernelGGL(k_call_post, dim3((unsigned)((k + 127) / 128)), dim3(128), 0, b->stream, (const ed_call*)b->d_calls.get(), k,
                     (const double*)b->d_loglik.get(), 3 * b->S, b->S, (int64_t)1, b->plan->d_lt3.get(), b->S, (const double*)b->req.post.d_beta.get(),
                     (const double*)b->req.post.d_logpost.get(), (const double*)b->req.post.d_logev.get(), b->req.d_cpost.get());
  HIP_TRY(hipGetLastError());
  if (timed) { HIP_TRY(ev.record(1, b->stream)); ev.live = true; }
  return ed_d2h(host_post, b->req.d_cpost, (size_t)k * sizeof(ed_call_post), b->stream);
}
ED_CATCH("ed_batch_copy_call_posterior")

// how many times the posterior passes have been enqueued on this batch since it was created (a request after the first launches nothing)
ED_EXPORT int64_t ed_batch_n_posterior_passes(const ed_batch* b) { return b ? b->req.post_passes : 0; }

// with ed_batch_enable_timing: the times of k_fb_backward, k_fb_forward and (if ed_batch_copy_call_posterior has been called since) k_call_post
// of the last run's posterior request, from events on its stream; 0 for what was not timed.  Synchronises that stream.
ED_EXPORT int ed_batch_posterior_ms(ed_batch* b, float ms[3])
try {
  if (!b || !ms) return ed_fail(ED_ERR_INVALID, "NULL argument");
  ms[2] = 0.f;
  if (int rc = request_ms(b, b->req.post_ev, 0, 1, &ms[0])) return rc;
  if (int rc = request_ms(b, b->req.post_ev, 1, 2, &ms[1])) return rc;
  return b->req.post_ev.live ? request_ms(b, b->req.cpost_ev, 0, 1, &ms[2]) : ED_OK;
}
ED_CATCH("ed_batch_posterior_ms")
