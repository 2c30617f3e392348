// edbins.inc -- depth-binned dispersion, `phi.bins > 1` of the ExomeDepth initialiser
// (reference R/class_definition.R:120-147), batched over the samples of an ed_batch.  Included by edcore.hip.
//
//   :124     ceiling.bin = quantile(reference, c(0.85, 1))          -> two order statistics per column by
//                                                                      bisection on the value (k_rs_count_le, k_rs_bisect)
//   :125-126 complete.bins = c(seq(0, q85, by = q85/(B-1)), max+1)   -> k_bins_edges
//   :127     depth.quant = #{edges <= reference}                    -> bins_group (in the fit kernels)
//   :130-133 every level must be populated                          -> group counts in k_fitb_moments, checked on the host
//   :135-139 aod::betabin(~ 1, random = ~ depth.quant)              -> k_fitb_* (Newton on eta, lambda_1..lambda_B:
//                                                                      arrow Hessian, Schur complement)
//   :141-147 phi.linear = approxfun(bin mid-points, phi)(reference)  -> bins_phi_linear (in k_emit_bins)
//   :184-189 get_loglike_matrix(phi.linear, expected, ...)           -> k_emit_bins: per-exon phi, so the three
//                                                                      lbeta(a1, a2) are per cell too (6 log-Betas)
// Parity: the emission arithmetic is that of k_emit_rows (bit-identical to the checker given phi per exon);
// the fit stands in for aod::betabin (not in the reference tree: parity unpinned, tolerance-level against
// oracle/edo_fit.inc::edo_fit_mle_groups).  This mode is functional, not tuned: one thread per cell, no route
// binning, no overlap of the Viterbi with the emissions.

namespace {

constexpr int kMaxPhiBins = 8;

// column maxima of the reference counts: partial[chunk][0][S] (then k_bins_max_reduce); bounds the bisection
__global__ void __launch_bounds__(kWave * kFitSub)
k_bins_colmax(const int32_t* __restrict__ ref, int64_t E, int64_t S, int32_t* __restrict__ pmax, const int* __restrict__ skip_from, int64_t T)
{
  // skip_from (the cohort reference sets: column = prefix * T + test): the columns from a test's first skipped prefix on are not needed
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  if (skip_from && (int)(s / T) >= skip_from[s % T]) { pmax[chunk * S + s] = 0; return; }
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  int32_t m = 0;
  int64_t e = e0;
  for (; e + 8 <= e1; e += 8) {       // (eight rows in flight)
    int32_t x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = ref[(e + u) * S + s];
#pragma unroll
    for (int u = 0; u < 8; ++u) m = max(m, x[u]);
  }
  for (; e < e1; ++e) m = max(m, ref[e * S + s]);
  pmax[chunk * S + s] = m;
}

__global__ void k_bins_max_reduce(const int32_t* __restrict__ pmax, int64_t nchunk, int64_t S, int32_t* __restrict__ xmax)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int32_t m = 0;
  for (int64_t c = 0; c < nchunk; ++c) m = max(m, pmax[c * S + s]);
  xmax[s] = m;
}

// bisection brackets [0, max] for both order statistics
__global__ void k_bins_bisect_init(const int32_t* __restrict__ xmax, int64_t S, int32_t* __restrict__ lo0, int32_t* __restrict__ hi0,
                                   int32_t* __restrict__ mid0, int32_t* __restrict__ lo1, int32_t* __restrict__ hi1,
                                   int32_t* __restrict__ mid1)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int32_t m = xmax[s];
  lo0[s] = 0; hi0[s] = m; mid0[s] = m / 2;
  lo1[s] = 0; hi1[s] = m; mid1[s] = m / 2;
}

__global__ void k_bins_edges(const int32_t* __restrict__ x_lo, const int32_t* __restrict__ x_hi,
                             const int32_t* __restrict__ x_max, double h, int B, int64_t S, double* __restrict__ edges)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double xl = (double)x_lo[s], xh = (double)x_hi[s];
  double q = xl;                                        // quantile type 7
  if (h > 0.0 && xh != xl) q = (1.0 - h) * xl + h * xh;
  const double by = q / (double)(B - 1);
  for (int k = 0; k < B; ++k) edges[(int64_t)k * S + s] = fmin((double)k * by, q);   // seq(): from + k*by, pmin(., to)
  edges[(int64_t)B * S + s] = (double)x_max[s] + 1.0;
}

// 0-based level of depth.quant: edges[0] = 0 <= x always, edges[B] > max
template <int B>
__device__ __forceinline__ int bins_group(double x, const double (&ed)[B])
{
  int g = 0;
#pragma unroll
  for (int k = 1; k < B; ++k) g += (x >= ed[k]) ? 1 : 0;
  return g;
}

// pooled moments for the starting point (as k_fit_moments) + the population of every level (all exons)
//   partial[chunk][q][S]: q = 0..3 sum y, sum n, sum y^2/n, #(n > 0);  q = 6 + g: exons in level g
template <int B>
__global__ void __launch_bounds__(kWave * kFitSub)
k_fitb_moments(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t E, int64_t S,
               const double* __restrict__ edges, double* __restrict__ partial)
{
  constexpr int Q = 6 * B;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  double ed[B];
#pragma unroll
  for (int k = 0; k < B; ++k) ed[k] = edges[(int64_t)k * S + s];
  double sy = 0, sn = 0, syy = 0, cnt = 0, pop[B];
#pragma unroll
  for (int g = 0; g < B; ++g) pop[g] = 0;
  for (int64_t e = e0; e < e1; ++e) {
    const int y = test[e * S + s], r = ref[e * S + s];
    const int n = y + r;
    if (n > 0) {
      sy += (double)y; sn += (double)n;
      syy += ((double)y * (double)y) / (double)n;
      cnt += 1.0;
    }
    const int g = bins_group<B>((double)r, ed);
#pragma unroll
    for (int gg = 0; gg < B; ++gg) pop[gg] += (g == gg) ? 1.0 : 0.0;
  }
  double* o = partial + (chunk * Q) * S + s;
  o[0] = sy; o[S] = sn; o[2 * S] = syy; o[3 * S] = cnt; o[4 * S] = 0; o[5 * S] = 0;
#pragma unroll
  for (int g = 0; g < B; ++g) o[(6 + g) * S] = pop[g];
#pragma unroll
  for (int q = 6 + B; q < Q; ++q) o[q * S] = 0;
}

// total of quantity q over the chunks, for 64 samples, in a fixed order (64 x kRedY threads, as reduce_partials)
__device__ __forceinline__ double bins_reduce_one(const double* __restrict__ partial, int64_t nchunk, int Q, int q, int64_t S,
                                                  int64_t s, bool live, double (*lds)[kWave])
{
  const int y = threadIdx.y, lane = threadIdx.x;
  double acc = 0.0;
  if (live)
    for (int64_t c = y; c < nchunk; c += kRedY) acc += partial[(c * Q + q) * S + s];
  __syncthreads();   // the previous quantity's readers are done with lds
  lds[y][lane] = acc;
  __syncthreads();
  for (int h = kRedY / 2; h >= 1; h >>= 1) {
    if (y < h) lds[y][lane] += lds[y + h][lane];
    __syncthreads();
  }
  return lds[0][lane];
}

// start: pooled method of moments for eta and every lambda_g; pop[g][s] for the host's level check
__global__ void __launch_bounds__(kWave * kRedY)
k_fitb_start(const double* __restrict__ partial, int64_t nchunk, int B, int64_t S, double* __restrict__ eta,
             double* __restrict__ lam, int* __restrict__ done, double* __restrict__ pop)
{
  __shared__ double lds[kRedY][kWave];
  const int Q = 6 * B;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool live = s < S;
  const double sy = bins_reduce_one(partial, nchunk, Q, 0, S, s, live, lds);
  const double sn = bins_reduce_one(partial, nchunk, Q, 1, S, s, live, lds);
  const double syy = bins_reduce_one(partial, nchunk, Q, 2, S, s, live, lds);
  const double cnt = bins_reduce_one(partial, nchunk, Q, 3, S, s, live, lds);
  for (int g = 0; g < B; ++g) {
    const double pg = bins_reduce_one(partial, nchunk, Q, 6 + g, S, s, live, lds);
    if (live && threadIdx.y == 0) pop[(int64_t)g * S + s] = pg;
  }
  if (!live || threadIdx.y != 0) return;
  double p = (sn > 0) ? sy / sn : 0.5;
  p = fmin(fmax(p, 1e-6), 1.0 - 1e-6);
  const double q = 1.0 - p;
  const double pearson = (syy - 2.0 * p * sy + p * p * sn) / (p * q);
  double phi = (sn - cnt > 0) ? (pearson - cnt) / (sn - cnt) : 0.01;
  phi = fmin(fmax(phi, 1e-4), 0.3);
  eta[s] = ed_plog(p / q);
  for (int g = 0; g < B; ++g) lam[(int64_t)g * S + s] = ed_plog((1.0 - phi) / phi);
  done[s] = (cnt < 2.0) ? 1 : 0;
}

// gradient / Hessian sums per level: partial[chunk][6 g + (ga, gb, haa, hab, hbb, cnt)][S]
template <int B>
__global__ void __launch_bounds__(kWave * kFitSub)
k_fitb_accum(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t E, int64_t S, int stride,
             const double* __restrict__ edges, const double* __restrict__ eta, const double* __restrict__ lam,
             const int* __restrict__ done, double* __restrict__ partial)
{
  constexpr int Q = 6 * B;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  if (done[s]) return;
  const double p = 1.0 / (1.0 + ed_pexp(-eta[s]));
  double ed[B], th[B];
#pragma unroll
  for (int g = 0; g < B; ++g) {
    ed[g] = edges[(int64_t)g * S + s];
    th[g] = ed_pexp(lam[(int64_t)g * S + s]);
  }
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  double acc[B][6];
#pragma unroll
  for (int g = 0; g < B; ++g)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[g][q] = 0.0;
  for (int64_t e = e0; e < e1; e += stride) {
    const int y = test[e * S + s], r = ref[e * S + s];
    const int n = y + r;
    if (n <= 0) continue;
    const int g = bins_group<B>((double)r, ed);
    double thg = th[0];
#pragma unroll
    for (int gg = 1; gg < B; ++gg) thg = (g == gg) ? th[gg] : thg;
    edfit::Acc c = {0, 0, 0, 0, 0};
    edfit::accumulate_cell(c, thg * p, thg * (1.0 - p), thg, y, n);
#pragma unroll
    for (int gg = 0; gg < B; ++gg) {
      const bool m = (g == gg);
      acc[gg][0] += m ? c.ga : 0.0;  acc[gg][1] += m ? c.gb : 0.0;  acc[gg][2] += m ? c.haa : 0.0;
      acc[gg][3] += m ? c.hab : 0.0; acc[gg][4] += m ? c.hbb : 0.0; acc[gg][5] += m ? 1.0 : 0.0;
    }
  }
  double* o = partial + (chunk * Q) * S + s;
#pragma unroll
  for (int g = 0; g < B; ++g)
#pragma unroll
    for (int q = 0; q < 6; ++q) o[(g * 6 + q) * S] = acc[g][q];
}

// One Newton step on (eta, u_1..u_B); u_g = lambda_g, or psi_g = 1/(a_g + b_g) below psi = 5e-5 (see k_fit_update).
// The Hessian couples the u_g only through eta (an arrow matrix):  S = sum_g (h_ee,g - h_eu,g^2 / h_uu,g),
//   d_eta = -sum_g (g_e,g - h_eu,g g_u,g / h_uu,g) / S,   d_u,g = -(g_u,g + h_eu,g d_eta) / h_uu,g.
// Globalisation as in k_fitc_update (edcov.inc; a 949-exon, 7-level case of the randomised sweep ended 20 % off in p
// without it): where the matrix is not negative definite (some h_uu,g >= 0 or S >= 0) its diagonal is shifted by
// mu |diag| (Levenberg; mu = 1e-3 * 10^k) until it is; the displacement in (eta, lambda_1..B) is scaled as a whole to
// max-coordinate <= 1; and a point whose gradient along the displacement just taken is < -1/2 of what it was at the
// start of it (the maximum was overshot) is replaced by the half-way point.
// state: [2 (kMaxPhiBins + 1) + 2][S] = previous point, displacement, slope, step length (0 = none yet).
// (the step itself: one thread per sample; called by k_fitb_update after its reductions and, pass after pass inside one launch, by
// k_lh_newton of edbins_hist.inc)
__device__ __noinline__ void fitb_step(const double (*tot)[6], int B, int64_t S, int64_t s, double* __restrict__ eta,
                                       double* __restrict__ lam, double* __restrict__ state, int* __restrict__ done, double tol,
                                       int final_pass)
{
  constexpr int kM = kMaxPhiBins + 1;
  double* prev = state + s;
  double* pd = state + (int64_t)kM * S + s;
  double& psl = state[(int64_t)(2 * kM) * S + s];
  double& pstep = state[(int64_t)(2 * kM + 1) * S + s];
  const double eta0 = eta[s];
  const double p = 1.0 / (1.0 + ed_pexp(-eta0));
  const double q = 1.0 - p;
  double g_l[kMaxPhiBins], g_u[kMaxPhiBins], h_eu[kMaxPhiBins], h_uu[kMaxPhiBins], thv[kMaxPhiBins], lam0[kMaxPhiBins];
  bool in_psi[kMaxPhiBins];
  double g_e_all = 0.0, h_ee_all = 0.0;
  for (int g = 0; g < B; ++g) {
    double ga = tot[g][0], gb = tot[g][1], haa = tot[g][2], hab = tot[g][3], hbb = tot[g][4];
    const double cnt = tot[g][5];
    lam0[g] = lam[(int64_t)g * S + s];
    const double th = ed_pexp(lam0[g]);
    thv[g] = th;
    const double a = th * p, b = th * q;
    double pa, qa, pb, qb, pt, qt;
    edfit::digamma_trigamma(a, pa, qa);
    edfit::digamma_trigamma(b, pb, qb);
    edfit::digamma_trigamma(th, pt, qt);
    ga -= cnt * (pa - pt);
    gb -= cnt * (pb - pt);
    haa -= cnt * (qa - qt);
    hab += cnt * qt;
    hbb -= cnt * (qb - qt);
    const double ae = a * q, be = -b * p;
    const double g_e = ga * ae + gb * be;
    g_l[g] = ga * a + gb * b;
    const double h_ee = haa * ae * ae + 2.0 * hab * ae * be + hbb * be * be + (ga * a * q - gb * b * p) * (1.0 - 2.0 * p);
    const double h_el = haa * ae * a + hab * (ae * b + a * be) + hbb * be * b + ga * ae + gb * be;
    const double h_ll = haa * a * a + 2.0 * hab * a * b + hbb * b * b + ga * a + gb * b;
    in_psi[g] = (1.0 / th) < 5e-5;
    if (in_psi[g]) { g_u[g] = -th * g_l[g]; h_eu[g] = -th * h_el; h_uu[g] = th * th * (h_ll + g_l[g]); }
    else { g_u[g] = g_l[g]; h_eu[g] = h_el; h_uu[g] = h_ll; }
    g_e_all += g_e;
    h_ee_all += h_ee;
  }
  // (only a displacement that the linear model called uphill can be said to have overshot: one bent by the bounds may start
  // downhill, and then halving it for ever -- 20 passes in a case of tools/fuzz_bins.py -- finds nothing; 1e-9 in log-likelihood
  // units is below what the sums resolve)
  if (pstep > 1e-6) {
    double sl = g_e_all * pd[0];
    for (int g = 0; g < B; ++g) sl += g_l[g] * pd[(int64_t)(1 + g) * S];
    if ((psl > 1e-9 && sl < -0.5 * psl) || !(sl == sl)) {   // overshot (or left the domain): half the displacement from the previous point
      const double st = 0.5 * pstep;
      pstep = st;
      eta[s] = prev[0] + st * pd[0];
      for (int g = 0; g < B; ++g) lam[(int64_t)g * S + s] = prev[(int64_t)(1 + g) * S] + st * pd[(int64_t)(1 + g) * S];
      return;
    }
  }
  // A level whose dispersion sits on its lower bound while the likelihood still rises towards 0 (an under-dispersed level: few
  // exons, low depth) is held there and leaves the system: kept in, its non-negative curvature made every step a shifted
  // (Levenberg) one, the other levels then converged linearly and the 40 passes ran out ~1e-4 short (tools/fuzz_bins.py).
  // A level where the likelihood is not concave in its own dispersion (far from its optimum, typically on the way down to the
  // bound) leaves the system as well, for this pass, and moves along its gradient by a fixed factor: shifting the whole matrix for
  // its sake (round 2) slowed every level down to that level's pace.
  bool pinned[kMaxPhiBins], loose[kMaxPhiBins];
  bool any_loose = false;
  for (int g = 0; g < B; ++g) {
    pinned[g] = in_psi[g] && (1.0 / thv[g] <= 1.0000001e-6) && (g_u[g] < 0.0);
    loose[g] = !pinned[g] && !(h_uu[g] < 0.0);
    any_loose = any_loose || loose[g];
  }
  double mu = 0.0, schur = 0.0, rhs = 0.0;
  bool ok = false;
  for (int tr = 0; tr < 12 && !ok; ++tr) {
    ok = true;
    schur = h_ee_all - mu * (fabs(h_ee_all) + 1e-300);
    rhs = g_e_all;
    for (int g = 0; g < B; ++g) {
      if (pinned[g] || loose[g]) continue;
      const double huu = h_uu[g] - mu * (fabs(h_uu[g]) + 1e-300);
      if (!(huu < 0.0)) { ok = false; break; }
      schur -= h_eu[g] * h_eu[g] / huu;
      rhs -= h_eu[g] * g_u[g] / huu;
    }
    if (ok && !(schur < 0.0)) ok = false;
    if (!ok) mu = (mu == 0.0) ? 1e-3 : mu * 10.0;
  }
  const bool newton = ok && mu == 0.0 && !any_loose;
  double de = ok ? -rhs / schur : g_e_all / (fabs(h_ee_all) + 1e-300);
  if (!(de == de)) de = 0.0;
  // displacement in (eta, lambda): a step in psi is converted (lambda = -log psi), with the same limits as k_fit_update
  double dl[kMaxPhiBins];
  double big = fabs(de);
  bool all_floor = true;
  for (int g = 0; g < B; ++g) {
    const double psi = 1.0 / thv[g];
    double du = ok ? -(g_u[g] + h_eu[g] * de) / (h_uu[g] - mu * (fabs(h_uu[g]) + 1e-300)) : g_u[g] / (fabs(h_uu[g]) + 1e-300);
    if (!(du == du) || pinned[g]) du = 0.0;
    if (loose[g]) du = in_psi[g] ? ((g_u[g] > 0.0) ? 0.65 * psi : -0.63 * psi) : ((g_u[g] > 0.0) ? 0.5 : -0.5);
    double npsi = in_psi[g] ? psi + du : psi * ed_pexp(-fmin(fmax(du, -2.0), 2.0));
    npsi = fmin(fmax(npsi, 0.1 * psi), 10.0 * psi);
    npsi = fmin(fmax(npsi, 1e-6), 2.0);
    dl[g] = -ed_plog(npsi) - lam0[g];
    big = fmax(big, fabs(dl[g]));
    if (!(npsi <= 1e-6 && psi <= 1.0000001e-6)) all_floor = false;
  }
  const double sc = (big > 1.0) ? 1.0 / big : 1.0;
  const double eta1 = fmin(fmax(eta0 + sc * de, -20.0), 20.0);
  de = eta1 - eta0;
  bool all_small = fabs(de) < tol;
  double slope = g_e_all * de;
  prev[0] = eta0; pd[0] = de;
  eta[s] = eta1;
  for (int g = 0; g < B; ++g) {
    const double d = sc * dl[g];
    const double psi = 1.0 / thv[g];
    if (!(fabs(d) < tol || psi <= 1.0000001e-6)) all_small = false;
    prev[(int64_t)(1 + g) * S] = lam0[g];
    pd[(int64_t)(1 + g) * S] = d;
    lam[(int64_t)g * S + s] = lam0[g] + d;
    slope += g_l[g] * d;
  }
  psl = slope;
  pstep = 1.0;
  // (a pass over a subset of the exons moves the iterate, it cannot declare convergence)
  if (final_pass && ((newton && all_small) || all_floor)) done[s] = 1;
}

__global__ void __launch_bounds__(kWave * kRedY)
k_fitb_update(const double* __restrict__ partial, int64_t nchunk, int B, int64_t S, double* __restrict__ eta,
              double* __restrict__ lam, double* __restrict__ state, int* __restrict__ done, double tol, int final_pass)
{
  __shared__ double lds[kRedY][kWave];
  const int Q = 6 * B;
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool live = (s < S) && !done[s < S ? s : 0];
  if (!__syncthreads_or(live ? 1 : 0)) return;
  double tot[kMaxPhiBins][6];
  for (int g = 0; g < B; ++g)
    for (int q = 0; q < 6; ++q) tot[g][q] = bins_reduce_one(partial, nchunk, Q, g * 6 + q, S, s, live, lds);
  if (!live || threadIdx.y != 0) return;
  fitb_step(tot, B, S, s, eta, lam, state, done, tol, final_pass);
}

// between the passes over every 16th exon and the passes over all of them: the overshoot test compares gradients of the
// same sums, so the displacement remembered from the last coarse pass is dropped
__global__ void k_fitb_forget_step(int64_t S, double* __restrict__ state)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) state[(int64_t)(2 * (kMaxPhiBins + 1) + 1) * S + s] = 0.0;
}

// Start of the grouped iteration: the converged intercept-only fit (one dispersion), every level at that dispersion.
__global__ void k_fitb_from_plain(const double* __restrict__ eta1, const double* __restrict__ lam1, int B, int64_t S,
                                  double* __restrict__ eta, double* __restrict__ lam, double* __restrict__ state)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  eta[s] = eta1[s];
  for (int g = 0; g < B; ++g) lam[(int64_t)g * S + s] = lam1[s];
  state[(int64_t)(2 * (kMaxPhiBins + 1) + 1) * S + s] = 0.0;   // no displacement taken yet
}

__global__ void k_fitb_finish(const double* __restrict__ eta, const double* __restrict__ lam, int B, int64_t S,
                              double* __restrict__ phi_bins, double* __restrict__ expected)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (int g = 0; g < B; ++g) phi_bins[(int64_t)g * S + s] = 1.0 / (ed_pexp(lam[(int64_t)g * S + s]) + 1.0);
  expected[s] = 1.0 / (1.0 + ed_pexp(-eta[s]));
}

// approxfun(x = bin mid-points, y = phi.estimates, yleft = y[1], yright = y[B])(v)  -- R's approx1, linear
__device__ __forceinline__ double bins_phi_linear(double v, int B, int64_t S, int64_t s, const double* __restrict__ edges,
                                                  const double* __restrict__ phib)
{
  // x[g] = (complete.bins[g] + complete.bins[g+1]) / 2, strictly increasing; y[g] = phi.estimates[g]
  double xi = (edges[s] + edges[S + s]) / 2;
  double yi = phib[s];
  if (v < xi) return yi;                                  // yleft
  for (int g = 1; g < B; ++g) {
    const double xg = (edges[(int64_t)g * S + s] + edges[(int64_t)(g + 1) * S + s]) / 2;
    const double yg = phib[(int64_t)g * S + s];
    if (v < xg) {                                         // x[g-1] <= v < x[g]
      if (v == xi) return yi;
      return yi + (yg - yi) * ((v - xi) / (xg - xi));
    }
    xi = xg; yi = yg;
  }
  return yi;                                              // v == x[B-1], or beyond it: yright = y[B-1]
}

// emissions with per-exon dispersion: the arithmetic of k_emit_rows per (exon, sample) cell -- six log-Betas, three
// of (a1 + obs, a2 + tot - obs) and three of (a1, a2) -- binned by evaluation route through LDS exactly as
// k_emit_batch does (a workgroup owns 4 exons x 64 samples = 1536 tasks)
constexpr int kBinTasks = kEmitBlock * 6;

// one tile (exon block `blk`, sample block `bx`) of k_emit_bins; workgroup-uniform control flow around the barriers
__device__ __forceinline__ void emit_bins_tile(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int B, const double* __restrict__ edges,
            const double* __restrict__ phib, const double* __restrict__ expected, const double* __restrict__ X, int K,
            const double* __restrict__ beta, double mixture, int64_t E, int64_t S, double* __restrict__ loglik,
            unsigned long long* __restrict__ nerr, const double* __restrict__ ctab, int rtab, const uint8_t* __restrict__ left_out,
            int64_t bx, int64_t blk, int64_t gx, const double* __restrict__ mix_s)
{
  // B > 0: phi interpolated from the depth levels (phib = phi.estimates); B == 0: phib = one phi per sample.
  // K >= 0: expected = plogis(X beta) per exon (edcov.inc); K < 0: `expected` holds one value per sample.
  // ctab != NULL: k_emit_bins_tab has done every cell whose three lbeta(a1, a2) are tabulated; this launch only does the
  // others (reference count beyond the table, or an entry that is not a finite number) -- whole workgroups without such a
  // cell return at once.
  __shared__ double t_a[kBinTasks];   // min (ratio route) or x; overwritten by the result
  __shared__ double t_b[kBinTasks];   // max (ratio route) or y
  __shared__ double t_r[kBinTasks];   // min/max
  __shared__ int n_front, n_back;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (tid == 0) { n_front = 0; n_back = 0; }
  __syncthreads();
  const int64_t s = bx * 64 + lane;
  const int64_t e = blk * (kEmitBlock / 64) + (tid >> 6);
  bool live = (e < E) && (s < S);
  if (ctab) {
    if (left_out[blk * gx + bx] == 0) return;   // uniform
    bool mine = false;
    if (live) {
      const int32_t r = ref[e * S + s];
      mine = ((unsigned)r >= (unsigned)rtab);
      if (!mine) {
        const double c0 = ctab[((int64_t)0 * rtab + r) * S + s], c1 = ctab[((int64_t)1 * rtab + r) * S + s], c2 = ctab[((int64_t)2 * rtab + r) * S + s];
        mine = !(fabs(c0) <= 1.7976931348623157e308 && fabs(c1) <= 1.7976931348623157e308 && fabs(c2) <= 1.7976931348623157e308);
      }
    }
    if (!__syncthreads_or(mine ? 1 : 0)) return;
    live = mine;
  }
  int slot[6];
  int nflag = 0;
  double a1[3], a2[3];
  int32_t obs = 0, tot = 0;
  {
    double phi = 0.5, ex = 0.5;
    if (live) {
      const int64_t cell = e * S + s;
      obs = test[cell];
      const int32_t r = ref[cell];
      tot = obs + r;                              // as.integer(reference + test), R/class_definition.R:187
      phi = (B > 0) ? bins_phi_linear((double)r, B, S, s, edges, phib) : phib[s];
      ex = (K >= 0) ? cov_expected(X, K, beta, e, S, s) : expected[s];
    }
    const double sd = __builtin_sqrt((phi * ex) * (1. - ex));
    double ep[3];
    state_props(ex, (mix_s && s < S) ? mix_s[s] : mixture, ep);   // mix_s: one mixture per sample (ed_batch_set_mixture)
#pragma unroll
    for (int st = 0; st < 3; ++st) shape_params(ep[st], sd, a1[st], a2[st]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int st = k >> 1;
    double x = 1.0, y = 1.0;
    if (live) {
      if (k & 1) { x = a1[st]; y = a2[st]; }
      else { x = a1[st] + (double)obs; y = (a2[st] + (double)tot) - (double)obs; }   // src/CNV_estimate.cpp:49
    }
    const bool pos = (x > 0.0 && y > 0.0);
    const double mx = (x > y ? x : y);
    const double mn = (x < y ? x : y);
    const double rat = mn / mx;
    const bool front = live && pos && (rat < 0.2);
    const bool back = live && !front;
    const unsigned long long mf = __ballot(front), mb = __ballot(back);
    const unsigned long long below = (1ull << lane) - 1ull;
    int basef = 0, baseb = 0;
    if (lane == 0) {
      basef = atomicAdd(&n_front, __popcll(mf));
      baseb = atomicAdd(&n_back, __popcll(mb));
    }
    basef = __shfl(basef, 0, 64);
    baseb = __shfl(baseb, 0, 64);
    int sl = 0;
    if (front) {
      sl = basef + __popcll(mf & below);
      t_a[sl] = mn; t_b[sl] = mx; t_r[sl] = rat;
    } else if (back) {
      sl = kBinTasks - 1 - (baseb + __popcll(mb & below));
      t_a[sl] = x; t_b[sl] = y; t_r[sl] = rat;
    }
    slot[k] = sl;
  }
  __syncthreads();
  const int nf = n_front, nb = n_back;
#pragma unroll 1
  for (int r = 0; r < 6; ++r) {
    const int sl = r * kEmitBlock + tid;
    if (sl < nf) {
      t_a[sl] = edsf::lnbeta_ratio(t_a[sl], t_b[sl], t_r[sl]);
    } else if (sl >= kBinTasks - nb) {
      const double x = t_a[sl], y = t_b[sl];
      int flag = 0;
      t_a[sl] = (x > 0.0 && y > 0.0) ? edsf::lnbeta_general(x, y) : edsf::lnbeta_cold(x, y, &flag);
      nflag += flag;
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int st = 0; st < 3; ++st) loglik[(e * 3 + st) * S + s] = t_a[slot[2 * st]] - t_a[slot[2 * st + 1]];
  }
  if (nflag) atomicAdd(nerr, (unsigned long long)nflag);
}

// grid (sample blocks, ceil(exon blocks / tiles_per_wg)): a workgroup walks `tiles_per_wg` consecutive exon blocks of its sample
// block.  1 for the launches that do every cell; 32 behind k_emit_bins_tab, where all but a few tiles return on their left_out byte
// (one workgroup per tile was 800 000 workgroups launched to read one byte each: 0.55 ms per slab).
__global__ void __launch_bounds__(kEmitBlock)
k_emit_bins(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int B, const double* __restrict__ edges,
            const double* __restrict__ phib, const double* __restrict__ expected, const double* __restrict__ X, int K,
            const double* __restrict__ beta, double mixture, int64_t E, int64_t S, double* __restrict__ loglik,
            unsigned long long* __restrict__ nerr, const double* __restrict__ ctab, int rtab, const uint8_t* __restrict__ left_out,
            const int* __restrict__ skip, int tiles_per_wg, int64_t n_blk, const double* __restrict__ mix_s)
{
  if (skip && *skip) return;
  const int64_t wg = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
  for (int t = 0; t < tiles_per_wg; ++t) {
    const int64_t blk = wg * tiles_per_wg + t;
    if (blk >= n_blk) break;
    emit_bins_tile(test, ref, B, edges, phib, expected, X, K, beta, mixture, E, S, loglik, nerr, ctab, rtab, left_out, (int64_t)blockIdx.x, blk,
                   (int64_t)gridDim.x, mix_s);
    __syncthreads();   // the tile's readers are done with the shared arrays
  }
}

// Per-exon dispersion makes the three lbeta(a1, a2) of a cell per-cell quantities -- but phi.linear is a function of the
// REFERENCE COUNT of the cell alone (approxfun(...)(reference), R/class_definition.R:141-147), an integer: for a sample and a
// state, lbeta(a1, a2) takes one value per distinct reference count.  ctab[st][r][s] = lbeta(a1, a2) for r < rtab, by the very
// functions the per-cell kernel calls (same bits); an entry that is not a finite number (shape parameters outside the positive
// quadrant: phi >= 1 ...) means "not tabulated" and sends its cells to the per-cell kernel, which also counts their GSL errors.
__global__ void __launch_bounds__(256)
k_bins_ctab(int B, const double* __restrict__ edges, const double* __restrict__ phib, const double* __restrict__ expected, double mixture,
            int64_t S, int rtab, double* __restrict__ ctab, const int* __restrict__ skip, const double* __restrict__ mix_s)
{
  if (skip && *skip) return;
  const int64_t s = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (s >= S || r >= rtab) return;
  const double phi = bins_phi_linear((double)r, B, S, s, edges, phib);
  const double ex = expected[s];
  const double sd = __builtin_sqrt((phi * ex) * (1. - ex));
  double ep[3];
  state_props(ex, mix_s ? mix_s[s] : mixture, ep);
#pragma unroll 1
  for (int st = 0; st < 3; ++st) {
    double a1, a2;
    shape_params(ep[st], sd, a1, a2);
    int flag = 0;
    const double c = (a1 > 0.0 && a2 > 0.0) ? edsf::lnbeta(a1, a2, &flag) : ed_pm_nan();
    ctab[((int64_t)st * rtab + r) * S + s] = c;
  }
}

// Emissions of the depth-binned model with the constants tabulated: three tasks per cell instead of six, binned by evaluation
// route through LDS as in k_emit_batch.  Cells without a table entry are left to k_emit_bins (launched afterwards).
constexpr int kBinTabTasks = kEmitBlock * 3;
__global__ void __launch_bounds__(kEmitBlock)
k_emit_bins_tab(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int B, const double* __restrict__ edges,
                const double* __restrict__ phib, const double* __restrict__ expected, double mixture, int64_t E, int64_t S,
                const double* __restrict__ ctab, int rtab, double* __restrict__ loglik, uint8_t* __restrict__ left_out,
                const int* __restrict__ skip, int64_t blk0, int64_t nblk, const double* __restrict__ mix_s)
{
  if (skip && *skip) return;
  // (the launch may be one of several pieces of the exon-block range: [blk0, blk0 + nblk))
  const int64_t blk_local = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (blk_local >= nblk) return;
  const int64_t blk = blk0 + blk_local;
  __shared__ double t_a[kBinTabTasks];   // min; overwritten by the result
  __shared__ double t_b[kBinTabTasks];   // max
  __shared__ double t_r[kBinTabTasks];   // min/max
  __shared__ double s_logt[ED_PM_LOGT_N * 3];
  __shared__ int n_front, n_back;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (tid == 0) { n_front = 0; n_back = 0; }
  {
    const double* __restrict__ flat = &k_logt_rows[0][0];
    s_logt[tid] = flat[tid];
    if (tid < ED_PM_LOGT_N * 3 - kEmitBlock) s_logt[kEmitBlock + tid] = flat[kEmitBlock + tid];
  }
  const int64_t s = (int64_t)blockIdx.x * 64 + lane;
  const int64_t e = blk * (kEmitBlock / 64) + (tid >> 6);
  const bool in = (e < E) && (s < S);
  int slot[3] = {-1, -1, -1};
  double cst[3] = {0, 0, 0};
  bool live = false;
  double tmn[3], tmx[3], tr[3];
  bool posv[3] = {false, false, false};
  if (in) {
    const int64_t cell = e * S + s;
    const int32_t obs = test[cell];
    const int32_t r = ref[cell];
    const int32_t tot = obs + r;                              // as.integer(reference + test), R/class_definition.R:187
    if ((unsigned)r < (unsigned)rtab) {
#pragma unroll
      for (int st = 0; st < 3; ++st) cst[st] = ctab[((int64_t)st * rtab + r) * S + s];
      live = fabs(cst[0]) <= 1.7976931348623157e308 && fabs(cst[1]) <= 1.7976931348623157e308 && fabs(cst[2]) <= 1.7976931348623157e308;
    }
    if (live) {
      const double phi = bins_phi_linear((double)r, B, S, s, edges, phib);
      const double ex = expected[s];
      const double sd = __builtin_sqrt((phi * ex) * (1. - ex));
      double ep[3];
      state_props(ex, mix_s ? mix_s[s] : mixture, ep);
#pragma unroll
      for (int st = 0; st < 3; ++st) {
        double a1, a2;
        shape_params(ep[st], sd, a1, a2);
        const double x = a1 + (double)obs, y = (a2 + (double)tot) - (double)obs;   // src/CNV_estimate.cpp:49
        posv[st] = (x > 0.0 && y > 0.0);
        tmn[st] = __builtin_fmin(x, y);
        tmx[st] = __builtin_fmax(x, y);
        tr[st] = tmn[st] / tmx[st];
      }
      // a finite table entry means a1, a2 > 0; obs >= 0 and tot >= obs keep x, y positive unless a count is negative:
      // such a cell goes to the per-cell kernel as well
      if (!(posv[0] && posv[1] && posv[2])) live = false;
    }
  }
  // one byte per workgroup: does it leave a cell to the per-cell kernel?  (that kernel's workgroups have the same shape and
  // return at once on a zero, without reading a count or a table entry)
  {
    const int any = __syncthreads_or((in && !live) ? 1 : 0);
    if (tid == 0) left_out[blk * gridDim.x + blockIdx.x] = (uint8_t)(any ? 1 : 0);
  }
  unsigned long long mf[3], mb[3];
  bool frontv[3];
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    frontv[st] = live && (tr[st] < 0.2);
    mf[st] = ed_ballot(frontv[st]);
    mb[st] = ed_ballot(live && !frontv[st]);
  }
  {
    const int nf0 = __popcll(mf[0]), nf1 = __popcll(mf[1]), nb0 = __popcll(mb[0]), nb1 = __popcll(mb[1]);
    int basef = 0, baseb = 0;
    if (lane == 0) {
      basef = atomicAdd(&n_front, nf0 + nf1 + __popcll(mf[2]));
      baseb = atomicAdd(&n_back, nb0 + nb1 + __popcll(mb[2]));
    }
    basef = __builtin_amdgcn_readfirstlane(basef);
    baseb = __builtin_amdgcn_readfirstlane(baseb);
    if (live) {
#pragma unroll
      for (int st = 0; st < 3; ++st) {
        const int offf = basef + (st > 0 ? nf0 : 0) + (st > 1 ? nf1 : 0);
        const int offb = (kBinTabTasks - 1) - (baseb + (st > 0 ? nb0 : 0) + (st > 1 ? nb1 : 0));
        const int sl = frontv[st] ? offf + ed_rank(mf[st]) : offb - ed_rank(mb[st]);
        t_a[sl] = tmn[st]; t_b[sl] = tmx[st]; t_r[sl] = tr[st];
        slot[st] = sl;
      }
    }
  }
  __syncthreads();
  const int nf = n_front, nb = n_back;
#pragma unroll 1
  for (int r = 0; r < 3; ++r) {
    const int sl = r * kEmitBlock + tid;
    if (sl < nf) {
      t_a[sl] = edsf::lnbeta_ratio_pre(t_a[sl], t_b[sl], t_r[sl], ed_pm_nan(), ed_pm_nan(), s_logt);
    } else if (sl >= kBinTabTasks - nb) {
      t_a[sl] = edsf::lnbeta_general_pre(t_a[sl], t_b[sl], ed_pm_nan(), s_logt);   // symmetric in (x, y)
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int st = 0; st < 3; ++st) loglik[(e * 3 + st) * S + s] = t_a[slot[st]] - cst[st];
  }
}

__global__ void k_bins_phi_linear(const int32_t* __restrict__ ref, int B, const double* __restrict__ edges,
                                  const double* __restrict__ phib, int64_t E, int64_t S, double* __restrict__ out)
{
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= E * S) return;
  const int64_t e = cell / S, s = cell - e * S;
  out[cell] = bins_phi_linear((double)ref[cell], B, S, s, edges, phib);
}

template <int B>
void fitb_launch_moments(dim3 grid, dim3 block, hipStream_t st, const int32_t* t, const int32_t* r, int64_t E, int64_t S,
                         const double* edges, double* partial)
{
  hipLaunchKernelGGL(k_fitb_moments<B>, grid, block, 0, st, t, r, E, S, edges, partial);
}
template <int B>
void fitb_launch_accum(dim3 grid, dim3 block, hipStream_t st, const int32_t* t, const int32_t* r, int64_t E, int64_t S, int stride,
                       const double* edges, const double* eta, const double* lam, const int* done, double* partial)
{
  hipLaunchKernelGGL(k_fitb_accum<B>, grid, block, 0, st, t, r, E, S, stride, edges, eta, lam, done, partial);
}

#include "edbins_hist.inc"

#define ED_BINS_DISPATCH(B, CALL)          \
  switch (B) {                             \
    case 2: CALL(2); break;                \
    case 3: CALL(3); break;                \
    case 4: CALL(4); break;                \
    case 5: CALL(5); break;                \
    case 6: CALL(6); break;                \
    case 7: CALL(7); break;                \
    default: CALL(8); break;               \
  }

// samples whose depth-binned Newton has not met its tolerance: the device's convergence flags, counted on the host (synchronises `st`)
static int bins_count_undone(const int* d_done, int64_t S, hipStream_t st, int64_t* n)
{
  std::vector<int> hd((size_t)S);
  HIP_TRY(hipMemcpyAsync(hd.data(), d_done, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int64_t k = 0;
  for (int v : hd) k += (v == 0);
  *n = k;
  return ED_OK;
}

// The histogram form (edbins_hist.inc) in three pieces, so that the cohort pipeline (edcohort.inc) can issue a slab's fit without
// looking at it and settle later:
//   fit_bins_hist_issue    everything up to `passes` Newton passes (+ k_fitb_finish when `finish`), then the device flags, the
//                          convergence flags and the level populations on their way to pinned host memory and an event: no wait
//   fit_bins_hist_passes   more Newton passes
//   fit_bins_hist_status   waits for the event: 0 = converged, 1 = this form declined (a device flag says why), 2 = a sample has not
//                          converged in the passes issued; an empty level is the reference's stop("Binning did not happen properly")
void fit_bins_hist_passes(ed_batch* b, int B, const double* d_edges, hipStream_t st, int n)
{
  BinsWork& w = *b->binsw;
  const int64_t S = b->S;
  const dim3 gq((unsigned)((S + kLhS - 1) / kLhS)), bq(kLhS, kLhY);
  const dim3 gred((unsigned)((S + kWave - 1) / kWave)), bred(kWave, kRedY);
  // all n passes in ONE launch (a pass per launch, each followed by its update launch, was 28 dependent launches: 0.6 ms of gaps on an
  // idle device, and under the neighbouring slab's emission launch -- where every launch queues for a free CU -- the 3.5-ms fit took 16.8)
  (void)gred; (void)bred;
  hipLaunchKernelGGL(k_lh_newton, gq, bq, 0, st, w.lhist, w.rhist, w.sorted, w.lvl_start, S, B, d_edges, w.eta, w.lam, w.done, w.part, w.flags,
                     w.state, n, 1e-8);
}

int fit_bins_hist_results(ed_batch* b, int B, hipStream_t st)
{
  BinsWork& w = *b->binsw;
  const int64_t S = b->S;
  int* h_flags = w.host.as<int>();
  int* h_done = h_flags + 1;
  double* h_pop = (double*)(w.host.as<char>() + ((4 + (size_t)S * 4 + 7) / 8) * 8);
  HIP_TRY(hipMemcpyAsync(h_flags, w.flags, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_done, w.done, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_pop, w.pop, (size_t)B * S * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(w.ev, st));
  HIP_TRY(hipGetLastError());
  return ED_OK;
}

int fit_bins_hist_issue(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int B, double* d_phi_bins, double* d_edges,
                        double* d_expected, hipStream_t st, int passes, bool finish)
{
  const int64_t E = b->plan->E, S = b->S;
  const double index = 1.0 + (double)std::max<int64_t>(E - 1, 0) * 0.85;   // quantile type 7: order statistics lo-1, hi-1 (0-based)
  const int64_t lo = (int64_t)std::floor(index), hi = (int64_t)std::ceil(index);
  const double h = index - (double)lo;
  if (!b->binsw) {
    b->binsw.reset(new (std::nothrow) BinsWork);
    if (!b->binsw) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  }
  BinsWork& w = *b->binsw;
  if (int rc = w.alloc(E, S, B)) return rc;
  if (int rc = batch_fitwork(b, E, S)) return rc;
  FitWork& fw = *b->fitw;
  const dim3 g1((unsigned)((S + 255) / 256)), b1(256);
  const dim3 gq((unsigned)((S + kLhS - 1) / kLhS)), bq(kLhS, kLhY);
  HIP_TRY(hipMemsetAsync(w.xmax, 0, (size_t)S * 4, st));
  HIP_TRY(hipMemsetAsync(w.beyond, 0, (size_t)S * 4, st));
  HIP_TRY(hipMemsetAsync(w.flags, 0, 4, st));
  HIP_TRY(hipMemsetAsync(w.done, 0, (size_t)S * 4, st));
  // ---- quantile(reference, c(0.85, 1)) and the edges ----
  hipLaunchKernelGGL(k_lh_rhist, dim3(lh_grid((S + kLhQS - 1) / kLhQS)), dim3(kLhBlock), 0, st, d_ref, E, S, w.rhist, w.xmax, w.beyond);
  hipLaunchKernelGGL(k_lh_select, gq, bq, 0, st, w.rhist, S, lo - 1, hi - 1, w.x0, w.x1, w.flags);
  hipLaunchKernelGGL(k_bins_edges, g1, b1, 0, st, w.x0, w.x1, w.xmax, h, B, S, d_edges);
  // ---- start: the converged single-dispersion fit, every level at that dispersion ----
  if (int rc = fit_columns(fw, FitJob::exon_major(d_test, d_ref, S).over(E, S).into(d_phi_bins, d_expected).by_method(1), st)) return rc;
  hipLaunchKernelGGL(k_fitb_from_plain, g1, b1, 0, st, fw.eta, fw.lam, B, S, w.eta, w.lam, w.state);
  // ---- per-level histograms, the lists, the populations ----
  const int KS = (B <= 3) ? 4 : (B <= 7) ? 2 : 1;
  const int nreg = kLhHalves * kLhBlock / KS, cap = kLhListTotal / nreg;
  const size_t lds = (size_t)KS * B * kLhK * 2;
  // (the attribute is per device and the call costs microseconds: set before every launch -- a process-wide "done" table was an unsynchronised
  //  read / write between the host threads of two pipelines on one device, and aliased devices beyond its 32 rows: ADVICE r5)
#define ED_LH_LAUNCH(KSV, SLOT)                                                                                                         \
  {                                                                                                                                     \
    HIP_TRY(hipFuncSetAttribute((const void*)k_lh_hist<KSV>, hipFuncAttributeMaxDynamicSharedMemorySize, 147456));                      \
    hipLaunchKernelGGL(k_lh_hist<KSV>, dim3(lh_grid((S + KSV - 1) / KSV)), dim3(kLhBlock), lds, st, d_test, d_ref, E, S, B, d_edges,   \
                       w.lhist, w.ov_y, w.ov_r, w.ovn, cap, w.flags);                                                                   \
  }
  if (KS == 4) ED_LH_LAUNCH(4, 0) else if (KS == 2) ED_LH_LAUNCH(2, 1) else ED_LH_LAUNCH(1, 2)
#undef ED_LH_LAUNCH
  hipLaunchKernelGGL(k_lh_lists, gq, bq, 0, st, w.ov_y, w.ov_r, w.ovn, cap, nreg, S, B, d_edges, w.rhist, w.beyond, w.sorted, w.lvl_start,
                     w.pop, w.flags);
  fit_bins_hist_passes(b, B, d_edges, st, passes);
  if (finish) hipLaunchKernelGGL(k_fitb_finish, g1, b1, 0, st, w.eta, w.lam, B, S, d_phi_bins, d_expected);
  return fit_bins_hist_results(b, B, st);
}

int fit_bins_hist_status(ed_batch* b, int B, int* status)
{
  BinsWork& w = *b->binsw;
  const int64_t S = b->S;
  HIP_TRY(hipEventSynchronize(w.ev));
  const int* h_flags = w.host.as<const int>();
  const int* h_done = h_flags + 1;
  const double* h_pop = (const double*)(w.host.as<const char>() + ((4 + (size_t)S * 4 + 7) / 8) * 8);
  *status = 0;
  if (*h_flags) { *status = 1; return ED_OK; }   // not this form's data
  for (int64_t s = 0; s < S; ++s)
    for (int g = 0; g < B; ++g)
      if (!(h_pop[(size_t)g * S + s] > 0))
        return ed_fail(ED_ERR_INVALID, "Binning did not happen properly (sample %lld: depth level %d of %d is empty)", (long long)s, g + 1, B);
  for (int64_t s = 0; s < S; ++s)
    if (!h_done[s]) { *status = 2; break; }
  return ED_OK;
}

// the synchronous entry's use of it: twelve passes are issued, then the flags are looked at; the other 28 of the budget only go out
// if a sample needs them.  *used = 0 on return: the data do not fit this form and nothing has been decided.
int fit_bins_hist(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int B, double* d_phi_bins, double* d_edges,
                  double* d_expected, hipStream_t st, int* used)
{
  *used = 0;
  if (int rc = fit_bins_hist_issue(b, d_test, d_ref, B, d_phi_bins, d_edges, d_expected, st, 12, false)) return rc;
  int status = 0;
  if (int rc = fit_bins_hist_status(b, B, &status)) return rc;
  if (status == 1) return ED_OK;
  if (status == 2) fit_bins_hist_passes(b, B, d_edges, st, 28);
  BinsWork& w = *b->binsw;
  hipLaunchKernelGGL(k_fitb_finish, dim3((unsigned)((b->S + 255) / 256)), dim3(256), 0, st, w.eta, w.lam, B, b->S, d_phi_bins, d_expected);
  HIP_TRY(hipGetLastError());
  b->bins_unconverged = 0;
  if (status == 2) { if (int rc = bins_count_undone(w.done, b->S, st, &b->bins_unconverged)) return rc; }
  *used = 1;
  return ED_OK;
}

}  // namespace

// Both workspace types are complete here.  The members go in reverse order of declaration: the workspaces, every buffer and event, the
// streams last (see the struct).
ed_batch::~ed_batch() = default;

ED_EXPORT int ed_batch_fit_bins(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int phi_bins, double* d_phi_bins,
                                double* d_edges, double* d_expected, void* stream_)
try {
  if (!b || !d_test || !d_ref || !d_phi_bins || !d_edges || !d_expected)
    return ed_fail(ED_ERR_INVALID, "ed_batch_fit_bins: NULL argument");
  if (b->counts_layout == 1) return ed_fail(ED_ERR_STATE, "ed_batch_fit_bins: the depth-binned model takes [n_exons][n_samples] counts (ed_batch_set_counts_layout(batch, 0))");
  if (phi_bins < 2 || phi_bins > kMaxPhiBins)
    return ed_fail(ED_ERR_INVALID, "ed_batch_fit_bins: phi_bins must be in 2..%d (phi.bins = 1 is ed_batch_fit)", kMaxPhiBins);
  hipStream_t st = (hipStream_t)stream_;
  const int64_t E = b->plan->E, S = b->S;
  const int B = phi_bins;
  if (E <= 0) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_bins: no exons");
  HIP_TRY(hipSetDevice(b->plan->device));
  b->fit_stream = st;
  if (b->timing) { if (int rc = fold_fit_time(b)) return rc; }
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[5], st));
  const int64_t nblk = (E + kFitChunk - 1) / kFitChunk, nchunk = nblk * kFitSub;
  const dim3 gcol((unsigned)((S + kWave - 1) / kWave), (unsigned)nblk), bcol(kWave, kFitSub);
  const dim3 gred((unsigned)((S + kWave - 1) / kWave)), bred(kWave, kRedY);
  const dim3 g1((unsigned)((S + 255) / 256)), b1(256);
  const double index = 1.0 + (double)std::max<int64_t>(E - 1, 0) * 0.85;
  const int64_t lo = (int64_t)std::floor(index), hi = (int64_t)std::ceil(index);
  const double h = index - (double)lo;
  b->bins_form = 0;
  if (b->fit_hist != 0) {   // (ed_batch_set_fit_histograms(batch, 0) asks for the per-cell form)
    int used = 0;
    if (int rc = fit_bins_hist(b, d_test, d_ref, B, d_phi_bins, d_edges, d_expected, st, &used)) return rc;
    b->bins_form = used;
    if (used) {
      if (b->timing) HIP_TRY(hipEventRecord(b->ev[6], st));
      b->have_fit_time = b->timing;
      HIP_TRY(hipStreamSynchronize(st));
      return ED_OK;
    }
  }
  DevBuf<void> dpart, dred, di32, deta, dlam, ddone, dpop, dstate;
  HIP_TRY(dpart.alloc((size_t)nchunk * 6 * B * S * 8));
  HIP_TRY(dred.alloc((size_t)kRsQ * S * 8));
  HIP_TRY(di32.alloc((size_t)7 * S * 4));
  HIP_TRY(deta.alloc((size_t)S * 8));
  HIP_TRY(dlam.alloc((size_t)B * S * 8));
  HIP_TRY(ddone.alloc((size_t)S * 4));
  HIP_TRY(dpop.alloc((size_t)B * S * 8));
  HIP_TRY(dstate.alloc((size_t)(2 * (kMaxPhiBins + 1) + 2) * S * 8));
  // ---- quantile(reference, c(0.85, 1)), type 7: order statistics lo-1, hi-1 (0-based) and E-1 ----
  int32_t* lo0 = di32.as<int32_t>(); int32_t* hi0 = lo0 + S; int32_t* mid0 = hi0 + S;
  int32_t* lo1 = mid0 + S; int32_t* hi1 = lo1 + S; int32_t* mid1 = hi1 + S;
  int32_t* xmax = mid1 + S;
  // the column maxima (= quantile(., 1)) first: they bound the bisection, which then needs ceil(log2(max + 1))
  // counting passes instead of 32
  DevBuf<void> dpmax;
  HIP_TRY(dpmax.alloc((size_t)nchunk * S * 4));
  hipLaunchKernelGGL(k_bins_colmax, gcol, bcol, 0, st, d_ref, E, S, dpmax.as<int32_t>(), (const int*)nullptr, (int64_t)1);
  hipLaunchKernelGGL(k_bins_max_reduce, g1, b1, 0, st, dpmax.as<int32_t>(), nchunk, S, xmax);
  int32_t gmax = 0;
  {
    std::vector<int32_t> hx((size_t)S);
    HIP_TRY(hipMemcpyAsync(hx.data(), xmax, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int32_t v : hx) gmax = std::max(gmax, v);
  }
  int steps = 1;
  while ((int64_t)1 << steps <= (int64_t)gmax) ++steps;   // brackets of width <= max + 1 close in `steps` halvings
  hipLaunchKernelGGL(k_bins_bisect_init, g1, b1, 0, st, xmax, S, lo0, hi0, mid0, lo1, hi1, mid1);
  for (int it = 0; it < steps + 1; ++it) {
    hipLaunchKernelGGL(k_rs_count_le, gcol, bcol, 0, st, d_ref, E, S, mid0, mid1, dpart.as<double>());
    hipLaunchKernelGGL(k_rs_reduce, gred, bred, 0, st, dpart.as<double>(), nchunk, S, dred.as<double>());
    hipLaunchKernelGGL(k_rs_bisect, g1, b1, 0, st, dred.as<double>(), S, lo - 1, hi - 1, lo0, hi0, mid0, lo1, hi1, mid1);
  }
  hipLaunchKernelGGL(k_bins_edges, g1, b1, 0, st, lo0, lo1, xmax, h, B, S, d_edges);
  // ---- fit ----
  double* part = dpart.as<double>();
  double* eta = deta.as<double>(); double* lam = dlam.as<double>(); int* done = ddone.as<int>();
#define ED_CALL_MOM(BB) fitb_launch_moments<BB>(gcol, bcol, st, d_test, d_ref, E, S, d_edges, part)
  ED_BINS_DISPATCH(B, ED_CALL_MOM)
#undef ED_CALL_MOM
  hipLaunchKernelGGL(k_fitb_start, gred, bred, 0, st, part, nchunk, B, S, eta, lam, done, dpop.as<double>());
  {
    // R/class_definition.R:130-133: every level of depth.quant must be populated
    std::vector<double> pop((size_t)B * S);
    HIP_TRY(hipMemcpyAsync(pop.data(), dpop.get(), pop.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t s = 0; s < S; ++s)
      for (int g = 0; g < B; ++g)
        if (!(pop[(size_t)g * S + s] > 0))
          return ed_fail(ED_ERR_INVALID, "Binning did not happen properly (sample %lld: depth level %d of %d is empty)",
                         (long long)s, g + 1, B);
  }
  // start from the converged single-dispersion fit (histogram form, ~1.6 ms): the levels' dispersions are corrections
  {
    if (int rc = batch_fitwork(b, E, S)) return rc;
    FitWork& w = *b->fitw;
    // (d_phi_bins' first row and d_expected serve as scratch outputs of the plain fit; both are rewritten below)
    if (int rc = fit_columns(w, FitJob::exon_major(d_test, d_ref, S).over(E, S).into(d_phi_bins, d_expected).by_method(1), st)) return rc;
    hipLaunchKernelGGL(k_fitb_from_plain, g1, b1, 0, st, w.eta, w.lam, B, S, eta, lam, dstate.as<double>());
  }
  // Newton from the converged single-dispersion fit: a few cheap passes over every 16th exon bring the levels' dispersions
  // within sampling error of their optimum (when there are enough exons for that), then passes over all exons; the budget is 40
  // full passes.  Ten are issued, then the convergence flags are looked at (this entry synchronises anyway) and the remaining
  // thirty only go out if a sample needs them.
  const int coarse = 0;   // measured at 200 000 x 1024, 3 levels: four coarse passes first do not save a full one (18.7 against 17.5 ms)
  for (int it = 0; it < coarse; ++it) {
#define ED_CALL_ACC(BB) fitb_launch_accum<BB>(gcol, bcol, st, d_test, d_ref, E, S, 16, d_edges, eta, lam, done, part)
    ED_BINS_DISPATCH(B, ED_CALL_ACC)
#undef ED_CALL_ACC
    hipLaunchKernelGGL(k_fitb_update, gred, bred, 0, st, part, nchunk, B, S, eta, lam, dstate.as<double>(), done, 1e-8, 0);
  }
  if (coarse) hipLaunchKernelGGL(k_fitb_forget_step, g1, b1, 0, st, S, dstate.as<double>());
  for (int it = 0; it < 40; ++it) {
    if (it == 10) {
      std::vector<int> hd((size_t)S);
      HIP_TRY(hipMemcpyAsync(hd.data(), done, (size_t)S * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      bool all = true;
      for (int v : hd) all = all && (v != 0);
      if (all) break;
    }
#define ED_CALL_ACC(BB) fitb_launch_accum<BB>(gcol, bcol, st, d_test, d_ref, E, S, 1, d_edges, eta, lam, done, part)
    ED_BINS_DISPATCH(B, ED_CALL_ACC)
#undef ED_CALL_ACC
    hipLaunchKernelGGL(k_fitb_update, gred, bred, 0, st, part, nchunk, B, S, eta, lam, dstate.as<double>(), done, 1e-8, 1);
  }
  hipLaunchKernelGGL(k_fitb_finish, g1, b1, 0, st, eta, lam, B, S, d_phi_bins, d_expected);
  HIP_TRY(hipGetLastError());
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[6], st));
  b->have_fit_time = b->timing;
  if (int rc = bins_count_undone(done, S, st, &b->bins_unconverged)) return rc;   // (synchronises: the work buffers above are released on return)
  return ED_OK;
}
ED_CATCH("ed_batch_fit_bins")

ED_EXPORT int ed_batch_fit_bins_n_unconverged(const ed_batch* b, int64_t* n)
try {
  if (!b || !n) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_bins_n_unconverged: NULL argument");
  *n = b->bins_unconverged;
  return ED_OK;
}
ED_CATCH("ed_batch_fit_bins_n_unconverged")

ED_EXPORT int ed_batch_fit_bins_form(const ed_batch* b) { return b ? b->bins_form : 0; }

ED_EXPORT int ed_batch_phi_linear(ed_batch* b, const int32_t* d_ref, int phi_bins, const double* d_phi_bins,
                                  const double* d_edges, double* d_phi_out, void* stream_)
try {
  if (!b || !d_ref || !d_phi_bins || !d_edges || !d_phi_out) return ed_fail(ED_ERR_INVALID, "ed_batch_phi_linear: NULL argument");
  if (b->counts_layout == 1) return ed_fail(ED_ERR_STATE, "ed_batch_phi_linear: the depth-binned model takes [n_exons][n_samples] counts (ed_batch_set_counts_layout(batch, 0))");
  if (phi_bins < 2 || phi_bins > kMaxPhiBins) return ed_fail(ED_ERR_INVALID, "ed_batch_phi_linear: phi_bins must be in 2..%d", kMaxPhiBins);
  const int64_t E = b->plan->E, S = b->S;
  if (E * S > 0)
    hipLaunchKernelGGL(k_bins_phi_linear, dim3((unsigned)((E * S + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, d_ref, phi_bins,
                       d_edges, d_phi_bins, E, S, d_phi_out);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}
ED_CATCH("ed_batch_phi_linear")

// ed_batch_fit_bins without the host's look at the result (the cohort pipeline settles it later: fit_bins_hist_status), and the run
// that follows it: its emission kernels return at once if the histogram form has declined (*skip != 0)
static int batch_fit_bins_async(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int phi_bins, double* d_phi_bins, double* d_edges,
                                double* d_expected, hipStream_t st)
{
  if (phi_bins < 2 || phi_bins > kMaxPhiBins) return ed_fail(ED_ERR_INVALID, "phi_bins must be in 2..%d", kMaxPhiBins);
  if (b->plan->E <= 0) return ed_fail(ED_ERR_INVALID, "ed_batch_fit_bins: no exons");
  HIP_TRY(hipSetDevice(b->plan->device));
  b->fit_stream = st;
  if (b->timing) { if (int rc = fold_fit_time(b)) return rc; }
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[5], st));
  if (int rc = fit_bins_hist_issue(b, d_test, d_ref, phi_bins, d_phi_bins, d_edges, d_expected, st, 14, true)) return rc;
  b->bins_form = 1;
  if (b->timing) HIP_TRY(hipEventRecord(b->ev[6], st));
  b->have_fit_time = b->timing;
  return ED_OK;
}
static int batch_run_bins_skip(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int phi_bins, const double* d_phi_bins,
                               const double* d_edges, const double* d_expected, double mixture, hipStream_t st)
{
  EmitModel em;
  em.bins = phi_bins; em.edges = d_edges;
  em.skip = b->binsw ? b->binsw->flags.get() : nullptr;
  return batch_run_impl(b, d_test, d_ref, d_phi_bins, d_expected, mixture, (void*)st, em);
}

ED_EXPORT int ed_batch_run_bins(ed_batch* b, const int32_t* d_test, const int32_t* d_ref, int phi_bins, const double* d_phi_bins,
                                const double* d_edges, const double* d_expected, double mixture, void* stream_)
try {
  if (!d_edges) return ed_fail(ED_ERR_INVALID, "ed_batch_run_bins: NULL argument");
  if (phi_bins < 2 || phi_bins > kMaxPhiBins) return ed_fail(ED_ERR_INVALID, "ed_batch_run_bins: phi_bins must be in 2..%d", kMaxPhiBins);
  EmitModel em;
  em.bins = phi_bins; em.edges = d_edges;
  return batch_run_impl(b, d_test, d_ref, d_phi_bins, d_expected, mixture, stream_, em);
}
ED_CATCH("ed_batch_run_bins")
