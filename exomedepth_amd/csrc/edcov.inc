// edcov.inc -- covariates in the mean model: `new('ExomeDepth', data = ..., formula = 'cbind(test, reference) ~ x1 + ...')`
// (reference R/class_definition.R:86-118, :168): aod::betabin fits one coefficient per column of the model matrix
// (logit link) and one dispersion; `expected` = fitted(mod) = plogis(X beta) is then per exon.  Included by edcore.hip.
//
//   logit p_e = beta_0 + sum_k beta_k x_ek,  a_e = p_e th,  b_e = (1 - p_e) th,  th = (1 - phi)/phi = exp(lambda)
//   Newton on (beta_0..beta_K, lambda): per cell the derivatives of lbeta(a_e + y, b_e + r) - lbeta(a_e, b_e) with
//   respect to (a, b) (digamma / trigamma DIFFERENCES, as in the histogram kernel), chain rule to (eta_e, lambda),
//   outer products with the covariate row for the (K+2) x (K+2) Hessian; deterministic two-stage reductions.
// The covariates are per exon and shared by the samples of the batch (X: double [E][K], exon-major), which is how
// GC content / exon length are used.  K <= kMaxCov.  Emissions: k_emit_bins with a per-cell `expected`.
// Parity: the fit stands in for aod::betabin (unpinned; tolerance-level against oracle edo_fit_mle_cov); the
// likelihood is bit-identical to the checker fed the same per-exon expected.

namespace {

constexpr int kMaxCov = 3;
constexpr int kCovM = kMaxCov + 2;                       // parameters: beta_0..beta_K, lambda
constexpr int kCovQ = kCovM + kCovM * (kCovM + 1) / 2;   // gradient + upper triangle of the Hessian = 20 (for K = kMaxCov)

__device__ __forceinline__ int cov_tri(int r, int c) { return r * kCovM - r * (r - 1) / 2 + (c - r); }   // r <= c

template <int K>
__global__ void __launch_bounds__(kWave * kFitSub)
k_fitc_accum(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, const double* __restrict__ X, int64_t E, int64_t S,
             const double* __restrict__ par /* [kCovM][S]: beta_0..beta_K, (unused), lambda at row K+1 */,
             const int* __restrict__ done, double* __restrict__ partial)
{
  constexpr int M = K + 2;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  if (done[s]) return;
  double beta[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) beta[k] = par[(int64_t)k * S + s];
  const double th = ed_pexp(par[(int64_t)(K + 1) * S + s]);
  double xt, rt, qt;
  edfit::digamma_trigamma_nolog(th, xt, rt, qt);
  const double ixt = edfit::frcp(xt);
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  double g[M], H[M * (M + 1) / 2];
#pragma unroll
  for (int i = 0; i < M; ++i) g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < M * (M + 1) / 2; ++i) H[i] = 0.0;
  for (int64_t e = e0; e < e1; ++e) {
    const int y = test[e * S + s], r = ref[e * S + s];
    const int n = y + r;
    if (n <= 0) continue;
    double x[K + 1];
    x[0] = 1.0;
    double eta = beta[0];
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k + 1] = X[e * K + k]; eta += beta[k + 1] * x[k + 1]; }
    const double p = 1.0 / (1.0 + ed_pexp(-eta)), q = 1.0 - p;
    const double a = th * p, b = th * q;
    double x1, r1, q1, x2, r2, q2, x3, r3, q3, xa, ra, qa, xb, rb, qb;
    edfit::digamma_trigamma_nolog(a + (double)y, x1, r1, q1);
    edfit::digamma_trigamma_nolog(b + (double)r, x2, r2, q2);
    edfit::digamma_trigamma_nolog(th + (double)n, x3, r3, q3);
    edfit::digamma_trigamma_nolog(a, xa, ra, qa);
    edfit::digamma_trigamma_nolog(b, xb, rb, qb);
    const double dt = edfit::flog(x3 * ixt) + (r3 - rt);                   // psi(th + n) - psi(th)
    const double A = (edfit::flog(x1 * edfit::frcp(xa)) + (r1 - ra)) - dt;  // d/da
    const double B = (edfit::flog(x2 * edfit::frcp(xb)) + (r2 - rb)) - dt;  // d/db
    const double Haa = (q1 - qa) - (q3 - qt), Hab = -(q3 - qt), Hbb = (q2 - qb) - (q3 - qt);
    const double ae = a * q, be = -b * p;
    const double ge = A * ae + B * be, gl = A * a + B * b;
    const double hee = Haa * ae * ae + 2.0 * Hab * ae * be + Hbb * be * be + (A * a * q - B * b * p) * (1.0 - 2.0 * p);
    const double hel = Haa * ae * a + Hab * (ae * b + a * be) + Hbb * be * b + A * ae + B * be;
    const double hll = Haa * a * a + 2.0 * Hab * a * b + Hbb * b * b + A * a + B * b;
    int t = 0;
#pragma unroll
    for (int i = 0; i <= K; ++i) {
      g[i] += ge * x[i];
#pragma unroll
      for (int j = i; j <= K; ++j) H[t++] += hee * x[i] * x[j];
      H[t++] += hel * x[i];
    }
    g[K + 1] += gl;
    H[t] += hll;
  }
  double* o = partial + (chunk * kCovQ) * S + s;
#pragma unroll
  for (int i = 0; i < M; ++i) o[(int64_t)i * S] = g[i];
#pragma unroll
  for (int i = 0; i < M * (M + 1) / 2; ++i) o[(int64_t)(kCovM + i) * S] = H[i];
}

// Newton step on (beta, lambda): solve H d = -g (Cholesky of -H); the step is taken if
// the Hessian is negative definite, a Levenberg-shifted step otherwise.  Globalisation (each was needed on
// cases the randomised sweep produced: large slopes make the first dispersion step overshoot, and clipping the
// coordinates one by one then turns the direction):
//   * the whole step vector is scaled so that its largest coordinate is <= 1 (the direction is kept);
//   * the point reached is checked by its directional derivative along the step just taken: g_new . d < -0.5 g_old . d
//     means the maximum along d was overshot -- the step is halved from the previous point instead (state: previous
//     point, d, g_old . d, current step length).
// phi is kept in [1e-6, 2/3].
__global__ void __launch_bounds__(kWave * kRedY)
k_fitc_update(const double* __restrict__ partial, int64_t nchunk, int K, int64_t S, double* __restrict__ par,
              double* __restrict__ state /* [2 kCovM + 2][S]: previous point, step, slope, step length (0 = none yet) */,
              int* __restrict__ done, double tol)
{
  __shared__ double lds[kRedY][kWave];
  const int M = K + 2;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool live = (s < S) && !done[s < S ? s : 0];
  if (!__syncthreads_or(live ? 1 : 0)) return;
  double g[kCovM], Hp[kCovM * (kCovM + 1) / 2];
  for (int i = 0; i < M; ++i) g[i] = bins_reduce_one(partial, nchunk, kCovQ, i, S, s, live, lds);
  for (int i = 0; i < M * (M + 1) / 2; ++i) Hp[i] = bins_reduce_one(partial, nchunk, kCovQ, kCovM + i, S, s, live, lds);
  if (!live || threadIdx.y != 0) return;
  double* prev = state + s;
  double* pd = state + (int64_t)kCovM * S + s;
  double& psl = state[(int64_t)(2 * kCovM) * S + s];
  double& pstep = state[(int64_t)(2 * kCovM + 1) * S + s];
  if (pstep > 1e-6) {
    double sl = 0.0;
    for (int i = 0; i < M; ++i) sl += g[i] * pd[(int64_t)i * S];
    if ((psl > 1e-9 && sl < -0.5 * psl) || !(sl == sl)) {   // overshot (or left the domain): half the step from the previous point
                                                              // (only an uphill displacement can overshoot: see k_fitb_update)
      const double st = 0.5 * pstep;
      pstep = st;
      for (int i = 0; i < M; ++i) par[(int64_t)i * S + s] = prev[(int64_t)i * S] + st * pd[(int64_t)i * S];
      return;
    }
  }
  // d = (-(H - mu D))^-1 g with D = diag|H|: mu = 0 is the Newton step; where the Hessian is not negative definite
  // (e.g. at the intercept-only optimum when a slope is strong: a saddle of the full model) the Cholesky factorisation
  // fails and mu is raised until it goes through (Levenberg's shift); past the ladder, the scaled gradient.
  double Hs[kCovM][kCovM], L[kCovM][kCovM], d[kCovM];
  {
    int t = 0;
    for (int i = 0; i < M; ++i)
      for (int j = i; j < M; ++j) { Hs[i][j] = Hp[t]; Hs[j][i] = Hp[t]; ++t; }
  }
  double mu = 0.0;
  bool ok = false;
  for (int tr = 0; tr < 12 && !ok; ++tr) {
    ok = true;
    for (int i = 0; i < M && ok; ++i) {
      for (int j = 0; j <= i; ++j) {
        double v = -Hs[i][j];
        if (i == j) v += mu * (fabs(Hs[i][i]) + 1e-300);
        for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
        if (i == j) {
          if (!(v > 0.0)) { ok = false; break; }
          L[i][i] = sqrt(v);
        } else {
          L[i][j] = v / L[j][j];
        }
      }
    }
    if (!ok) mu = (mu == 0.0) ? 1e-3 : mu * 10.0;
  }
  const bool newton = ok && mu == 0.0;
  if (ok) {
    for (int i = 0; i < M; ++i) {   // L z = g
      double v = g[i];
      for (int k = 0; k < i; ++k) v -= L[i][k] * d[k];
      d[i] = v / L[i][i];
    }
    for (int i = M - 1; i >= 0; --i) {   // L' d = z
      double v = d[i];
      for (int k = i + 1; k < M; ++k) v -= L[k][i] * d[k];
      d[i] = v / L[i][i];
    }
  } else {
    for (int i = 0; i < M; ++i) d[i] = g[i] / (fabs(Hs[i][i]) + 1e-300);
  }
  for (int i = 0; i < M; ++i) if (!(d[i] == d[i])) d[i] = 0.0;
  double slope;
  double big = 0.0;
  for (int i = 0; i < M; ++i) big = fmax(big, fabs(d[i]));
  if (big > 1.0) {
    const double sc = 1.0 / big;
    for (int i = 0; i < M; ++i) d[i] *= sc;
  }
  // the box: intercept and slopes in [-30, 30], phi in [1e-6, 2/3]
  slope = 0.0;
  for (int i = 0; i < M; ++i) {
    const double lo = (i == M - 1) ? -0.6931471805599453 : -30.0, hi = (i == M - 1) ? 13.815509557963773 : 30.0;
    const double x0 = par[(int64_t)i * S + s];
    const double x1 = fmin(fmax(x0 + d[i], lo), hi);
    d[i] = x1 - x0;
    prev[(int64_t)i * S] = x0;
    pd[(int64_t)i * S] = d[i];
    par[(int64_t)i * S + s] = x1;
    slope += d[i] * g[i];
  }
  psl = slope;
  pstep = 1.0;
  if (newton && big < tol) done[s] = 1;
}

__global__ void k_fitc_init(const double* __restrict__ eta, const double* __restrict__ lam, int K, int64_t S, double* __restrict__ par,
                            double* __restrict__ state, int* __restrict__ done)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double e0 = eta[s], l0 = lam[s];   // (par aliases nothing of the fit workspace)
  par[s] = e0;
  for (int k = 1; k <= K; ++k) par[(int64_t)k * S + s] = 0.0;
  par[(int64_t)(K + 1) * S + s] = l0;
  state[(int64_t)(2 * kCovM + 1) * S + s] = 0.0;   // no step taken yet
  done[s] = 0;                                       // every sample iterates again with its covariates
}

__global__ void k_fitc_finish(const double* __restrict__ par, int K, int64_t S, double* __restrict__ beta, double* __restrict__ phi)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (int k = 0; k <= K; ++k) beta[(int64_t)k * S + s] = par[(int64_t)k * S + s];
  phi[s] = 1.0 / (ed_pexp(par[(int64_t)(K + 1) * S + s]) + 1.0);
}

// fitted(mod) = plogis(X beta): the S4 `expected` slot, [E][S]
__global__ void k_cov_expected(const double* __restrict__ X, int K, const double* __restrict__ beta, int64_t E, int64_t S,
                               double* __restrict__ out)
{
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= E * S) return;
  const int64_t e = cell / S, s = cell - e * S;
  out[cell] = cov_expected(X, K, beta, e, S, s);
}

template <int K>
void fitc_launch_accum(dim3 grid, dim3 block, hipStream_t st, const int32_t* t, const int32_t* r, const double* X, int64_t E, int64_t S,
                       const double* par, const int* done, double* partial)
{
  hipLaunchKernelGGL(k_fitc_accum<K>, grid, block, 0, st, t, r, X, E, S, par, done, partial);
}

}  // namespace

ED_EXPORT int ed_batch_fit_cov(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, const double* d_X, int n_cov,
                               double* d_beta, double* d_phi, void* stream_)
try {
  if (!b || !d_test || !d_ref || !d_beta || !d_phi || (n_cov > 0 && !d_X)) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_cov: NULL argument");
  if (b->counts_layout == 1) return ed_fail(ED_ERR_STATE, "ed_batch_fit_cov: the covariate model takes [n_exons][n_samples] counts (ed_batch_set_counts_layout(batch, 0))");
  if (n_cov < 0 || n_cov > kMaxCov) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_cov: n_cov must be in 0..%d", kMaxCov);
  hipStream_t st = (hipStream_t)stream_;
  const int64_t E = b->plan->E, S = b->S;
  const int K = n_cov;
  if (E <= 0) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_cov: no exons");
  HIP_TRY(hipSetDevice(b->plan->device));
  b->fit_stream = st;
  if (b->timing) { if (int rc = fold_fit_time(b)) return rc; }
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[5], st));
  if (int rc = batch_fitwork(b, E, S)) return rc;
  FitWork& w = *b->fitw;
  const int64_t nblk = (E + kFitChunk - 1) / kFitChunk, nchunk = nblk * kFitSub;
  const dim3 gcol((unsigned)((S + kWave - 1) / kWave), (unsigned)nblk), bcol(kWave, kFitSub);
  const dim3 gred((unsigned)((S + kWave - 1) / kWave)), bred(kWave, kRedY);
  const dim3 g1((unsigned)((S + 255) / 256)), b1(256);
  DevBuf<void> dpart, dpar, dstate;
  HIP_TRY(dpart.alloc((size_t)nchunk * kCovQ * S * 8));
  HIP_TRY(dpar.alloc((size_t)kCovM * S * 8));
  HIP_TRY(dstate.alloc((size_t)(2 * kCovM + 2) * S * 8));
  // start: the converged intercept-only model (the histogram fit: robust from any start, ~1.6 ms), slopes 0 -- the
  // covariate effects are corrections, so the Newton iteration below begins inside its region of convergence.
  // (Started from the pooled moments it wandered off on a 953-exon case the randomised sweep produced.)
  if (int rc = fit_columns(w, FitJob::exon_major(d_test, d_ref, S).over(E, S).into(d_phi, dpar.as<double>() /* scratch: expected */).by_method(1), st)) return rc;
  hipLaunchKernelGGL(k_fitc_init, g1, b1, 0, st, w.eta, w.lam, K, S, dpar.as<double>(), dstate.as<double>(), w.done);
  for (int it = 0; it < 40; ++it) {
    switch (K) {
      case 0: fitc_launch_accum<0>(gcol, bcol, st, d_test, d_ref, d_X, E, S, dpar.as<double>(), w.done, dpart.as<double>()); break;
      case 1: fitc_launch_accum<1>(gcol, bcol, st, d_test, d_ref, d_X, E, S, dpar.as<double>(), w.done, dpart.as<double>()); break;
      case 2: fitc_launch_accum<2>(gcol, bcol, st, d_test, d_ref, d_X, E, S, dpar.as<double>(), w.done, dpart.as<double>()); break;
      default: fitc_launch_accum<3>(gcol, bcol, st, d_test, d_ref, d_X, E, S, dpar.as<double>(), w.done, dpart.as<double>()); break;
    }
    hipLaunchKernelGGL(k_fitc_update, gred, bred, 0, st, dpart.as<double>(), nchunk, K, S, dpar.as<double>(), dstate.as<double>(), w.done, 1e-8);
  }
  hipLaunchKernelGGL(k_fitc_finish, g1, b1, 0, st, dpar.as<double>(), K, S, d_beta, d_phi);
  HIP_TRY(hipGetLastError());
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[6], st));
  b->have_fit_time = b->timing;
  HIP_TRY(hipStreamSynchronize(st));   // the work buffers above are released on return
  return ED_OK;
}
ED_CATCH("ed_batch_fit_cov")

ED_EXPORT int ed_batch_run_cov(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, const double* d_X, int n_cov,
                               const double* d_beta, const double* d_phi, double mixture, void* stream_)
try {
  if (!d_beta || (n_cov > 0 && !d_X)) return ed_fail(ED_ERR_INVALID, "ed_batch_run_cov: NULL argument");
  if (n_cov < 0 || n_cov > kMaxCov) return ed_fail(ED_ERR_INVALID, "ed_batch_run_cov: n_cov must be in 0..%d", kMaxCov);
  EmitModel em;
  em.K = n_cov; em.X = d_X; em.beta = d_beta; em.cov = true;
  return batch_run_impl(b, d_test, d_ref, d_phi, d_beta /* stands for `expected` in the NULL checks */, mixture, stream_, em);
}
ED_CATCH("ed_batch_run_cov")

ED_EXPORT int ed_batch_expected_cov(ed_batch* b, const double* d_X, int n_cov, const double* d_beta, double* d_expected_out,
                                    void* stream_)
try {
  if (!b || !d_beta || !d_expected_out || (n_cov > 0 && !d_X)) return ed_fail(ED_ERR_INVALID, "ed_batch_expected_cov: NULL argument");
  if (n_cov < 0 || n_cov > kMaxCov) return ed_fail(ED_ERR_INVALID, "ed_batch_expected_cov: n_cov must be in 0..%d", kMaxCov);
  const int64_t E = b->plan->E, S = b->S;
  if (E * S > 0)
    hipLaunchKernelGGL(k_cov_expected, dim3((unsigned)((E * S + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, d_X, n_cov, d_beta, E, S,
                       d_expected_out);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}
ED_CATCH("ed_batch_expected_cov")
