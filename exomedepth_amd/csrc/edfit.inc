// edfit.inc -- the single-dispersion beta-binomial fit (K5) in one place, included by edcore.hip once: the per-cell kernels, the choice of histogram
// geometry, the three geometries of the histogram form (edfit_hist.inc), the column fit on tail counts (edfit_col.inc), the workspace FitWork and
// the driver fit_columns.  A fit is asked for with a FitJob (ed_fit_job.hpp, host only), which also holds the checks a request must pass before
// anything is enqueued.  What needs the complete ed_batch (batch_fitwork, ed_batch_fit*, the setters) is in edcore.hip; the other callers are
// edbins.inc, edcov.inc, edrefset.inc and edrefcohort.inc.
#include "ed_fit_job.hpp"
static_assert(kFitJobErrInvalid == ED_ERR_INVALID && kFitJobErrState == ED_ERR_STATE, "ed_fit_job.hpp restates the two error codes");

namespace {

// ---- K5: per-sample beta-binomial fit -------------------------------------------------------
// Exon axis cut into chunks of kFitChunk exons; thread = (sample lane, sub-chunk).  Every pass writes
// per-chunk partial sums [chunk][q][S] that the update kernel adds up in a fixed order, so the fit is
// reproducible run to run (no floating-point atomics).
constexpr int kFitSub = 4;          // sub-chunks (waves) per workgroup
constexpr int kFitChunk = 1024;     // exons per workgroup
constexpr int kFitQ = 6;            // quantities per partial

// moments for the starting point: sum y, sum n, sum y^2/n, #cells with n > 0
__global__ void __launch_bounds__(kWave * kFitSub)
k_fit_moments(const int32_t* __restrict__ test, int64_t trs, int64_t tcs, const int32_t* __restrict__ ref, int64_t rrs,
              int64_t E, int64_t S, int stride, double* __restrict__ partial, int64_t tmod)
{
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t ts = (tmod ? s % tmod : s) * tcs;   // tmod > 0: column s takes test column s mod tmod (edrefcohort.inc)
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  double sy = 0, sn = 0, syy = 0, cnt = 0;
  for (int64_t e = e0; e < e1; e += stride) {
    const int y = test[e * trs + ts];   // (trs, tcs) = (S, 1): one column per sample; (1, 0): one shared column
    const int n = y + ref[e * rrs + s];
    if (n > 0) {
      sy += (double)y; sn += (double)n;
      syy += ((double)y * (double)y) / (double)n;
      cnt += 1.0;
    }
  }
  double* o = partial + (chunk * kFitQ) * S + s;
  o[0] = sy; o[S] = sn; o[2 * S] = syy; o[3 * S] = cnt; o[4 * S] = 0; o[5 * S] = 0;
}

// k_fit_moments for sample-major counts ([S][E], `pitch` ints between samples): one workgroup per sample reads every `stride`-th
// 64-exon piece of its row (coalesced) and leaves its sums as chunk 0 of the partials (k_fit_start is then given one chunk).
// Exon e of the fit is element e * by of the row (by > 1: subset.for.speed).
__global__ void __launch_bounds__(256)
k_fit_moments_sm(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t pitch, int64_t by, int64_t E, int64_t S,
                 int stride, double* __restrict__ partial, double* __restrict__ eta, double* __restrict__ lam, int* __restrict__ done,
                 int* __restrict__ depth_max, int cb)
{
  __shared__ double red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s = blockIdx.x;
  const int64_t row0 = s * pitch;
  double sy = 0, sn = 0, syy = 0, cnt = 0;
  for (int64_t q = (int64_t)wave * stride; q * 64 < E; q += 4 * (int64_t)stride) {
    const int64_t e = q * 64 + lane;
    if (e < E) {
      const int y = ed_ldc(test, row0 + e * by, cb);
      const int n = y + ed_ldc(ref, row0 + e * by, cb);
      if (n > 0) {
        sy += (double)y; sn += (double)n;
        syy += ((double)y * (double)y) / (double)n;
        cnt += 1.0;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sy += __shfl_xor(sy, d, 64); sn += __shfl_xor(sn, d, 64); syy += __shfl_xor(syy, d, 64); cnt += __shfl_xor(cnt, d, 64);
  }
  if (lane == 0) { red[wave][0] = sy; red[wave][1] = sn; red[wave][2] = syy; red[wave][3] = cnt; }
  __syncthreads();
  if (tid < 4) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    partial[(int64_t)tid * S + s] = v;
  }
  if (tid == 4 || tid == 5) partial[(int64_t)tid * S + s] = 0.0;
  if (tid == 0) {     // k_fit_start's method-of-moments start for this sample (same arithmetic), saving its launch
    const double tsy = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], tsn = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    const double tsyy = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2], tcnt = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
    double p = (tsn > 0) ? tsy / tsn : 0.5;
    p = fmin(fmax(p, 1e-6), 1.0 - 1e-6);
    const double q = 1.0 - p;
    const double pearson = (tsyy - 2.0 * p * tsy + p * p * tsn) / (p * q);
    double phi = (tsn - tcnt > 0) ? (pearson - tcnt) / (tsn - tcnt) : 0.01;
    phi = fmin(fmax(phi, 1e-4), 0.3);
    eta[s] = ed_plog(p / q);
    lam[s] = ed_plog((1.0 - phi) / phi);
    done[s] = (tcnt < 2.0) ? 1 : 0;
    if (tcnt > 0) atomicMax(depth_max, (int)fmin(tsn / tcnt, 2.0e9));
  }
}

// Sum the per-chunk partials of one quantity set for 64 samples with a 64 x kRedY thread block: thread
// (lane, y) adds chunks y, y + kRedY, ... in order, then the kRedY strands are added in a fixed tree in
// LDS.  The order never depends on timing, so the fit is reproducible run to run.
constexpr int kRedY = 16;
__device__ __forceinline__ void reduce_partials(const double* __restrict__ partial, int64_t nchunk, int64_t S, int64_t s,
                                                bool live, double (&out)[kFitQ], double (*lds)[kRedY][kWave])
{
  const int y = threadIdx.y, lane = threadIdx.x;
  double acc[kFitQ];
#pragma unroll
  for (int q = 0; q < kFitQ; ++q) acc[q] = 0.0;
  if (live) {
    for (int64_t c = y; c < nchunk; c += kRedY) {
      const double* o = partial + (c * kFitQ) * S + s;
#pragma unroll
      for (int q = 0; q < kFitQ; ++q) acc[q] += o[q * S];
    }
  }
#pragma unroll
  for (int q = 0; q < kFitQ; ++q) lds[q][y][lane] = acc[q];
  __syncthreads();
  for (int h = kRedY / 2; h >= 1; h >>= 1) {
    if (y < h) {
#pragma unroll
      for (int q = 0; q < kFitQ; ++q) lds[q][y][lane] += lds[q][y + h][lane];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kFitQ; ++q) out[q] = lds[q][0][lane];
}

// method-of-moments start: p0 = sum y / sum n; phi0 from the Pearson statistic
//   sum_e (y - n p)^2 / (n p q) ~ cnt + phi * sum_e (n - 1)
__global__ void __launch_bounds__(kWave * kRedY)
k_fit_start(const double* __restrict__ partial, int64_t nchunk, int64_t S, double* __restrict__ eta,
            double* __restrict__ lam, int* __restrict__ done, int* __restrict__ depth_max)
{
  __shared__ double lds[kFitQ][kRedY][kWave];
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool live = s < S;
  double tot[kFitQ];
  reduce_partials(partial, nchunk, S, s, live, tot, lds);
  if (!live || threadIdx.y != 0) return;
  const double sy = tot[0], sn = tot[1], syy = tot[2], cnt = tot[3];
  double p = (sn > 0) ? sy / sn : 0.5;
  p = fmin(fmax(p, 1e-6), 1.0 - 1e-6);
  const double q = 1.0 - p;
  const double pearson = (syy - 2.0 * p * sy + p * p * sn) / (p * q);
  double phi = (sn - cnt > 0) ? (pearson - cnt) / (sn - cnt) : 0.01;
  phi = fmin(fmax(phi, 1e-4), 0.3);
  eta[s] = ed_plog(p / q);
  lam[s] = ed_plog((1.0 - phi) / phi);
  done[s] = (cnt < 2.0) ? 1 : 0;   // nothing to fit
  // the batch's depth (largest per-sample mean total): picks the histogram geometry, see fit_hist_geometry
  if (cnt > 0) atomicMax(depth_max, (int)fmin(sn / cnt, 2.0e9));
}

// select.reference.set for a cohort (edrefcohort.inc): column i * T + j is test j against its i + 1 best candidates summed, and the
// reference's loop stops at the first i + 1 > 2 whose fitted proportion is below 0.05 (R/optimize_reference_set.R:130) -- the
// prefixes after that are never looked at.  The proportion falls as references are added, and its moment estimate (sum y / sum n,
// the start value in eta) is within a few per cent of the fitted one: the columns after the first prefix whose moment estimate is
// below `p_limit` (0.04: 20 % of margin) are marked done before the Newton passes.  skip_from[j] = the first prefix skipped (K if
// none): the caller falls back to the slow path should the fitted loop ever reach it.
__global__ void k_fit_skip_prefixes(const double* __restrict__ eta, int* __restrict__ done, int K, int64_t T, double p_limit,
                                    int* __restrict__ skip_from)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= T) return;
  int from = K;
  for (int i = 0; i < K; ++i) {
    if (i >= from) { done[(int64_t)i * T + j] = 1; continue; }
    const double p = 1.0 / (1.0 + ed_pexp(-eta[(int64_t)i * T + j]));
    if (i + 1 > 2 && p < p_limit) from = i + 1;
  }
  skip_from[j] = from;
}

__global__ void __launch_bounds__(kWave * kFitSub)
k_fit_accum(const int32_t* __restrict__ test, int64_t trs, int64_t tcs, const int32_t* __restrict__ ref, int64_t rrs,
            int64_t E, int64_t S, int stride, const double* __restrict__ eta, const double* __restrict__ lam, const int* __restrict__ done,
            double* __restrict__ partial, int64_t tmod, const int32_t* __restrict__ colmap = nullptr, const int* __restrict__ n_map = nullptr)
{
  // colmap (late passes, k_fit_compact): slot j of the launch works on column colmap[j], j < *n_map -- the columns still iterating, packed.
  // A wave is as slow as its slowest lane: after the third full pass of the cohort reference sets' fit 10 % of the columns were still
  // iterating and 96 % of the waves with them; packed, the fourth pass costs a tenth.
  const int64_t j = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (colmap && j >= *n_map) return;
  const int64_t s = colmap ? (int64_t)colmap[j] : j;
  const int64_t ts = (tmod ? s % tmod : s) * tcs;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (s >= S) return;
  if (done[s]) return;
  const double th = ed_pexp(lam[s]);
  const double p = 1.0 / (1.0 + ed_pexp(-eta[s]));
  const double a = th * p, b = th * (1.0 - p);
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, E);
  edfit::Acc acc = {0, 0, 0, 0, 0};
  double cnt = 0;
  // (trs, tcs) = (S, 1): one test column per sample; (1, 0): one shared test column.
  // The counts of the next kPre cells are requested before the current ones are consumed: ~150 VALU
  // instructions per cell do not cover an HBM round trip on their own.
  constexpr int kPre = 8;      // cells of a column requested ahead of the one being consumed (round 5: 4 -> 8)
  int yb[kPre], rb[kPre];
#pragma unroll
  for (int k = 0; k < kPre; ++k) {
    const int64_t e = e0 + (int64_t)k * stride;
    yb[k] = (e < e1) ? test[e * trs + ts] : 0;
    rb[k] = (e < e1) ? ref[e * rrs + s] : 0;
  }
  for (int64_t e = e0; e < e1; e += (int64_t)kPre * stride) {
    int yc[kPre], rc[kPre];
#pragma unroll
    for (int k = 0; k < kPre; ++k) { yc[k] = yb[k]; rc[k] = rb[k]; }
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      const int64_t en = e + (int64_t)(kPre + k) * stride;
      yb[k] = (en < e1) ? test[en * trs + ts] : 0;
      rb[k] = (en < e1) ? ref[en * rrs + s] : 0;
    }
    // one logarithm per run of kPre cells and gradient component (ed_fit_dev.hpp: accumulate_cell_run); the short digamma / trigamma series when
    // THIS lane's arguments of the run are all large.  The choice is the lane's own: a wave-wide vote made a column's sums depend on which columns
    // shared its wave (k_fit_compact packs them in atomic order), and the two series differ in the last bits (tests/test_gpu_fit_invariance.py).
    // A wave with lanes of both kinds runs both branches.
    double small = 1e300;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      if (e + (int64_t)k * stride < e1 && yc[k] + rc[k] > 0) small = fmin(small, fmin(a + (double)yc[k], b + (double)rc[k]));
    }
    const bool big = small >= 32.0;                       // (th + n >= a + y)
    double pa = 1.0, pb = 1.0;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      if (e + (int64_t)k * stride < e1) {
        const int y = yc[k], n = yc[k] + rc[k];
        if (n > 0) cnt += 1.0;
        edfit::accumulate_cell_run(acc, pa, pb, a, b, th, y, n, big);
      }
    }
    acc.ga += edfit::flog(pa);
    acc.gb += edfit::flog(pb);
  }
  double* o = partial + (chunk * kFitQ) * S + j;       // (the partials of a packed pass sit at the slot, not at the column)
  o[0] = acc.ga; o[S] = acc.gb; o[2 * S] = acc.haa; o[3 * S] = acc.hab; o[4 * S] = acc.hbb; o[5 * S] = cnt;
}

// the columns still iterating, packed (order irrelevant): colmap[0 .. *n_map)
__global__ void k_fit_compact(const int* __restrict__ done, int64_t S, int32_t* __restrict__ colmap, int* __restrict__ n_map)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = s < S && !done[s];
  const unsigned long long m = __builtin_amdgcn_ballot_w64(act);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(n_map, __popcll(m));
  base = __builtin_amdgcn_readfirstlane(base);
  if (act) colmap[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)s;
}

// One Newton step on (eta, lambda) = (logit p, log(a+b)) from the summed gradient/Hessian of the log-likelihood
// with respect to (a, b) (tot = ga, gb, haa, hab, hbb, #cells, without the per-sample constant terms).  Steps are
// capped, and a non-concave local model falls back to a scaled gradient step.  `final_pass` marks passes over
// all exons: only those may declare convergence.
__device__ __forceinline__ void fit_newton_step(const double (&tot)[kFitQ], double& eta_v, double& lam_v, int& done_v, double tol,
                                                int final_pass)
{
  double ga = tot[0], gb = tot[1], haa = tot[2], hab = tot[3], hbb = tot[4], cnt = tot[5];
  const double th = ed_pexp(lam_v);
  const double p = 1.0 / (1.0 + ed_pexp(-eta_v));
  const double q = 1.0 - p;
  const double a = th * p, b = th * q;
  if (cnt != 0.0) {                                // (0: the caller's sums already hold the constant terms -- the histogram forms)
    double pa, qa, pb, qb, pt, qt;
    edfit::digamma_trigamma(a, pa, qa);
    edfit::digamma_trigamma(b, pb, qb);
    edfit::digamma_trigamma(th, pt, qt);
    ga -= cnt * (pa - pt);
    gb -= cnt * (pb - pt);
    haa -= cnt * (qa - qt);
    hab += cnt * qt;
    hbb -= cnt * (qb - qt);
  }
  const double ae = a * q, be = -b * p;          // d a / d eta, d b / d eta
  const double g_e = ga * ae + gb * be;
  const double g_l = ga * a + gb * b;
  const double h_ee = haa * ae * ae + 2.0 * hab * ae * be + hbb * be * be + (ga * a * q - gb * b * p) * (1.0 - 2.0 * p);
  const double h_el = haa * ae * a + hab * (ae * b + a * be) + hbb * be * b + ga * ae + gb * be;
  const double h_ll = haa * a * a + 2.0 * hab * a * b + hbb * b * b + ga * a + gb * b;
  // Dispersion coordinate of the Newton step.  lambda = log(a+b) is the better-conditioned coordinate for
  // ordinary dispersions (one full pass fewer than psi), but for nearly binomial data (phi -> 0) the
  // likelihood is exponentially flat in lambda and regular in psi = 1/(a+b) = phi/(1-phi), and a Newton
  // iteration in lambda walks off into the flat region: below psi = 5e-5 the step is taken in psi.
  // Chain rule:  d/dpsi = -th d/dlambda  =>  g_s = -th g_l,  h_es = -th h_el,  h_ss = th^2 (h_ll + g_l).
  const double psi = 1.0 / th;
  double de, ds;
  bool newton;   // a genuine Newton step (locally concave model): only such a step may declare convergence
  if (psi >= 5e-5) {
    const double det = h_ee * h_ll - h_el * h_el;
    double dl;
    newton = (h_ee < 0.0 && det > 0.0);
    if (newton) {
      de = -(h_ll * g_e - h_el * g_l) / det;
      dl = -(h_ee * g_l - h_el * g_e) / det;
    } else {
      // Not locally concave (typically psi far below its optimum, where the likelihood is convex and nearly flat
      // in lambda): move uphill in lambda by the Newton magnitude but at most 0.5 -- a factor 1.65 in psi -- per
      // iteration.  (A step scaled by the whole Hessian crawls: 1.4 % per iteration on the case kept in
      // tests/golden/fit_slow_start_case.npz.)
      de = g_e / (fabs(h_ee) + 1e-300);
      dl = (g_l > 0.0 ? 1.0 : -1.0) * fmin(0.5, fabs(g_l) / (fabs(h_ll) + 1e-300));
    }
    dl = fmin(fmax(dl, -1.0), 1.0);
    ds = psi * (ed_pexp(-dl) - 1.0);
  } else {
    const double g_s = -th * g_l;
    const double h_es = -th * h_el;
    const double h_ss = th * th * (h_ll + g_l);
    const double det = h_ee * h_ss - h_es * h_es;
    newton = (h_ee < 0.0 && det > 0.0);
    if (newton) {
      de = -(h_ss * g_e - h_es * g_s) / det;
      ds = -(h_ee * g_s - h_es * g_e) / det;
    } else {
      de = g_e / (fabs(h_ee) + 1e-300);
      ds = (g_s > 0.0 ? 1.0 : -1.0) * fmin(0.5 * psi, fabs(g_s) / (fabs(h_ss) + 1e-300));
    }
  }
  // Pinned at the lower bound of psi with the step pointing further down (nearly binomial data): psi stays, and the mean takes its
  // own one-dimensional Newton step -- it is what still has to converge (declared converged on reaching the bound, as rounds 1-3
  // did, a 36-row column kept an expected proportion 2 % off its maximum).
  const bool pinned = psi <= 1.0000001e-6 && ds <= 0.0;
  if (pinned) {
    newton = h_ee < 0.0;
    de = newton ? -g_e / h_ee : g_e / (fabs(h_ee) + 1e-300);
    ds = 0.0;
  }
  de = fmin(fmax(de, -1.0), 1.0);
  double npsi = psi + ds;
  npsi = fmin(fmax(npsi, 0.1 * psi), 10.0 * psi);       // multiplicative trust region
  // phi in [1e-6, 2/3].  Below phi ~ 1e-6 the model is numerically binomial: a + b > 1e6 and the digamma
  // differences that make up the gradient cancel to noise, so the dispersion is not estimable in binary64.
  npsi = fmin(fmax(npsi, 1e-6), 2.0);
  const double ne = fmin(fmax(eta_v + de, -20.0), 20.0);
  eta_v = ne;
  lam_v = -ed_plog(npsi);
  // Newton converges quadratically: once a step over ALL exons is below tol (kFitStepTol = 2e-5 in the per-cell passes, relative for psi), the
  // error left after applying it is of order C tol^2 = C 4e-10 against the 1e-8 the fit is held to -- no confirming pass is needed
  // (tests/test_gpu_fit.py::test_per_cell_fit_on_ill_conditioned_columns pins that margin on tiny-phi / few-exon columns).  (Pinned at the lower bound of psi: npsi = psi, and the test is the mean's.)
  if (final_pass && newton && fabs(de) < tol && fabs(npsi - psi) < tol * psi) done_v = 1;
}

__global__ void __launch_bounds__(kWave * kRedY)
k_fit_update(const double* __restrict__ partial, int64_t nchunk, int64_t S, double* __restrict__ eta,
             double* __restrict__ lam, int* __restrict__ done, double tol, int final_pass, const int32_t* __restrict__ colmap = nullptr,
             const int* __restrict__ n_map = nullptr)
{
  __shared__ double lds[kFitQ][kRedY][kWave];
  const int64_t j = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const bool in_map = !colmap || j < *n_map;
  const int64_t s = (colmap && in_map) ? (int64_t)colmap[j] : j;
  const bool live = in_map && (s < S) && !done[s < S ? s : 0];
  if (!__syncthreads_or(live ? 1 : 0)) return;   // the whole tile has converged
  double tot[kFitQ];
  reduce_partials(partial, nchunk, S, j, live, tot, lds);
  if (!live || threadIdx.y != 0) return;
  double e = eta[s], l = lam[s];
  int d = 0;
  fit_newton_step(tot, e, l, d, tol, final_pass);
  eta[s] = e; lam[s] = l;
  if (d) done[s] = 1;
}

// ---- K5 through count histograms --------------------------------------------------------------------
// The gradient and Hessian of the log-likelihood are sums over cells of psi / psi' at a + y, b + (n - y) and
// a + b + n: functions of ONE count each.  So they are sums over the distinct values of y, n - y and n weighted by
// how often each value occurs in the sample -- three histograms per sample, built in ONE pass over the counts
// (k_fit_hist: LDS-privatised, 8 / 4 / 2 samples per workgroup).  Every Newton iteration then costs one reciprocal per
// bin instead of 3 x n_exons digamma evaluations, and all iterations run inside one launch (k_fit_hnewton).  Cells
// with a count beyond the histogram range go to per-sample overflow lists (second-level bins in LDS, then one by
// one); a sample whose list runs out is summed cell by cell inside the same launch.
// (Sums are grouped by value instead of by exon: the result differs from the per-cell path by rounding only.)
// Which geometry serves a batch, and which of the launched ones runs: fit_hist_geometry and fit_hist_bit, shared with the host's choice of what
// to launch (ed_fit_job.hpp, where both are described).
__device__ __forceinline__ bool fit_hist_runs(int depth, int launched, int mine)
{
  const int sel = fit_hist_geometry(depth);
  if (launched & fit_hist_bit(sel)) return mine == sel;
  return mine == ((launched & 4) ? 2 : ((launched & 2) ? 4 : 8));
}

// what a geometry's launches (edfit_hist.inc: Launch) take from fit_columns: the job, the workspace's buffers, the geometries launched
struct FitHistArgs {
  const FitJob& j;
  hipStream_t st;
  uint32_t* hist; int32_t* ov_y; int32_t* ov_r; int32_t* ovn;   // FitWork::HistSet
  const int64_t* cap;                                           // [3] cells per list, by geometry (Launch::kIndex)
  double* eta; double* lam; int* done; int* depth; int* fevals;
  int launched;
  // element (e, s) of the counts at e * cell_rs() + s * cell_cs()
  int64_t cell_rs() const { return j.sample_major() ? j.trs : j.rrs; }
  int64_t cell_cs() const { return j.sample_major() ? j.sm_pitch : 1; }
};

namespace hg8 {
#define ED_HG_KS 8
#include "edfit_hist.inc"
#undef ED_HG_KS
}
namespace hg4 {
#define ED_HG_KS 4
#include "edfit_hist.inc"
#undef ED_HG_KS
}
namespace hg2 {
#define ED_HG_KS 2
#include "edfit_hist.inc"
#undef ED_HG_KS
}

__global__ void k_fit_finish(const double* __restrict__ eta, const double* __restrict__ lam, int64_t S,
                             double* __restrict__ phi, double* __restrict__ expected)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double th = ed_pexp(lam[s]);
  phi[s] = 1.0 / (th + 1.0);                        // phi = 1/(a + b + 1)
  expected[s] = 1.0 / (1.0 + ed_pexp(-eta[s]));     // fitted(mod) = plogis(eta)
}
}  // namespace

#include "edfit_col.inc"

// The histogram form's buffers serve whichever geometry runs, in either layout, so each is sized for the largest:
constexpr int64_t kHistWords = (int64_t)hg2::kHistHalves * hg2::kHistK;   // `hist`, words per (padded) sample
constexpr int64_t kHistLists = hg2::kHistGroups;                          // `ovn`, counts per sample
constexpr bool hist_holds(int64_t halves, int64_t bins, int64_t sm_bins, int64_t lists)
{
  return halves * bins <= kHistWords     // k_fit_hist: [halves][quads][kHistK][4]
         && sm_bins <= kHistWords        // k_fit_hist_sm: one row of kSmBins per sample -- longer than kHistK where it holds the second level
         && lists <= kHistLists;         // a count per (list, sample)
}
static_assert(hist_holds(hg8::kHistHalves, hg8::kHistK, hg8::kSmBins, hg8::kHistGroups) && hist_holds(hg4::kHistHalves, hg4::kHistK, hg4::kSmBins, hg4::kHistGroups) &&
              hist_holds(hg2::kHistHalves, hg2::kHistK, hg2::kSmBins, hg2::kHistGroups), "every geometry fits the histogram buffers");

// workspace of the column-wise beta-binomial fit (shared by ed_batch_fit and ed_select_reference_set)
struct FitWork {
  DevBuf<double> partial;      // [nchunk][kFitQ][S]
  DevBuf<double> eta, lam;
  DevBuf<int> done;
  DevBuf<int32_t> colmap;      // [S] the columns still iterating after the third full pass, packed (k_fit_compact)
  DevBuf<int> n_map;           // ... their number
  DevBuf<int> fevals;          // fit mode 1: objective evaluations of each sample's Nelder-Mead search
  struct HistSet {             // the histogram form's buffers, made on its first use (alloc_hist): all four or none
    DevBuf<uint32_t> hist;     // count histograms (k_fit_hist; layout and size depend on the geometry, sized for the largest)
    DevBuf<int32_t> ov_y, ov_r;   // [lists][cap][S] cells beyond the histogram range, per row group of k_fit_hist
    DevBuf<int32_t> ovn;       // [lists][S] overflow cells of each (row group, sample)
    bool made() const { return (bool)hist; }
  } hs;
  DevBuf<int> depth;           // largest per-sample mean total of the columns being fitted (device; k_fit_start)
  PinBuf<int> h_depth;         // the same, copied back after every fit (pinned host memory): next call's hint, -1 = none yet
  int64_t cap[3] = {0, 0, 0};  // cells per list, by geometry (hgN::Launch::kIndex); set by alloc_hist
  int64_t nchunk = 0, S = 0, E_max = 0;
  struct HistBytes { size_t hist, ov, ovn; };   // ov: each of ov_y, ov_r
  HistBytes hist_bytes() const
  {
    // (the lists: cap x kHistGroups slots per sample in both layouts, [slot][S] and [S][slot] -- the largest product of the three geometries')
    const int64_t slots = std::max({cap[0] * hg8::kHistGroups, cap[1] * hg4::kHistGroups, cap[2] * hg2::kHistGroups});
    return HistBytes{(size_t)kHistWords * hg2::hist_padded(S) * 4, (size_t)slots * S * 4, (size_t)kHistLists * S * 4};
  }
  int alloc_hist()
  {
    if (hs.made()) return ED_OK;
    // sized for the largest fit this workspace serves
    cap[hg8::Launch::kIndex] = hg8::Launch::cap_of(E_max); cap[hg4::Launch::kIndex] = hg4::Launch::cap_of(E_max); cap[hg2::Launch::kIndex] = hg2::Launch::cap_of(E_max);
    const HistBytes n = hist_bytes();
    HistSet t;
    const bool ok = t.hist.alloc(n.hist) == hipSuccess && t.ov_y.alloc(n.ov) == hipSuccess && t.ov_r.alloc(n.ov) == hipSuccess &&
                    t.ovn.alloc(n.ovn) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return ed_fail(ED_ERR_NOMEM, "beta-binomial fit: cannot allocate the count histograms");
    }
    hs = std::move(t);
    return ED_OK;
  }
  int alloc(int64_t E, int64_t S_)
  {
    const int rc = alloc_impl(E, S_);
    if (rc != ED_OK) *this = FitWork();     // nothing half-allocated stays behind
    return rc;
  }
  int alloc_impl(int64_t E, int64_t S_)
  {
    *this = FitWork();
    S = S_;
    E_max = E;
    nchunk = ((E + kFitChunk - 1) / kFitChunk) * kFitSub;
    HIP_TRY(partial.alloc((size_t)std::max<int64_t>(nchunk, 1) * kFitQ * S * 8));
    // all-ones = NaN: a chunk read without having been written by the current fit shows up instead of passing as zero
    HIP_TRY(hipMemset(partial, 0xff, (size_t)std::max<int64_t>(nchunk, 1) * kFitQ * S * 8));
    HIP_TRY(eta.alloc((size_t)S * 8));
    HIP_TRY(lam.alloc((size_t)S * 8));
    HIP_TRY(done.alloc((size_t)S * 4));
    HIP_TRY(colmap.alloc((size_t)S * 4));
    HIP_TRY(n_map.alloc(4));
    HIP_TRY(fevals.alloc((size_t)S * 4));
    HIP_TRY(hipMemset(fevals, 0, (size_t)S * 4));
    HIP_TRY(ed_null_stream_fence());
    HIP_TRY(depth.alloc(4));
    HIP_TRY(h_depth.alloc(4));
    *h_depth = -1;
    return ED_OK;
  }
};

// Step below which a full pass of the per-cell form declares a column converged.  Newton converges quadratically (fit_newton_step): a
// step s leaves an error ~C s^2, and the fit is held to 1e-8 -- 2e-5 leaves ~4e-10 C.  Rounds 1-4 asked for 1e-6, which the third full
// pass met only barely (its step IS ~1e-6 from the stride-16 start): a fourth pass over most of the cohort reference sets' 32 768 columns,
// 1.5 of the leg's 9 ms, confirmed what was already there.
constexpr double kFitStepTol = 2e-5;
constexpr int kFitCoarsePasses = 4;   // Newton steps on every 16th exon before the full passes (1 / 16 of a full pass each)
// Serve one request (ed_fit_job.hpp).  hist != 0: build count histograms once and iterate on them in one launch (needs one test column per sample laid
// out like the reference counts: the exon-major and sample-major views); otherwise per-cell passes, one launch pair per pass.  A request that
// cannot be served is refused before anything is enqueued: the workspace and the caller's outputs are as they were.
static int fit_columns(FitWork& w, const FitJob& j, hipStream_t st)
{
  int code = ED_OK;
  if (const char* why = fitjob::invalid(j, w.E_max, w.S, &code)) return ed_fail(code, "%s", why);
  if (j.hist) { if (int rc = w.alloc_hist()) return rc; }
  const int64_t E = j.E, S = j.S;
  const bool sm = j.sample_major();
  const int64_t nblk = (E + kFitChunk - 1) / kFitChunk;
  const int64_t nch = sm ? 1 : nblk * kFitSub;   // chunks THIS fit writes (the workspace may have been sized for more exons)
  const dim3 grid((unsigned)((S + kWave - 1) / kWave), (unsigned)nblk), block(kWave, kFitSub);
  const dim3 g1((unsigned)((S + 255) / 256)), b1(256);
  const dim3 gr((unsigned)((S + kWave - 1) / kWave)), br(kWave, kRedY);
  // every pass rewrites all partials, so chunks a strided pass barely touches cannot leave stale sums
  // (fit mode 1 starts from aod's glm-binomial intercept logit(sum y / sum n) over ALL exons; the Newton fit only needs a rough start)
  const int mstride = j.mode == 1 ? 1 : (E >= 65536 ? 16 : 4);
  HIP_TRY(hipMemsetAsync(w.depth, 0, 4, st));
  if (sm) hipLaunchKernelGGL(k_fit_moments_sm, dim3((unsigned)S), dim3(256), 0, st, j.test, j.ref, j.sm_pitch, j.trs, E, S, mstride, w.partial,
                             w.eta, w.lam, w.done, w.depth, j.cb);
  else {
    hipLaunchKernelGGL(k_fit_moments, grid, block, 0, st, j.test, j.trs, j.tcs, j.ref, j.rrs, E, S, mstride, w.partial, j.tmod);
    hipLaunchKernelGGL(k_fit_start, gr, br, 0, st, w.partial, nch, S, w.eta, w.lam, w.done, w.depth);
  }
  if (j.hist) {
    if (const char* poison = getenv("ED_FIT_POISON")) {     // (diagnostic) the histogram workspace starts every fit from a byte pattern: a result that depends on what
      const int byte = atoi(poison) & 0xff;                // the allocation happened to hold differs with the pattern -- ED_FIT_POISON=165, =0, =255 ...
      const FitWork::HistBytes n = w.hist_bytes();
      HIP_TRY(hipMemsetAsync(w.hs.hist, byte, n.hist, st));
      HIP_TRY(hipMemsetAsync(w.hs.ov_y, byte, n.ov, st));
      HIP_TRY(hipMemsetAsync(w.hs.ov_r, byte, n.ov, st));
      HIP_TRY(hipMemsetAsync(w.hs.ovn, byte, n.ovn, st));
    }
    // Which geometries to launch: the one asked for (tests), else the one the previous fit's depth points to, else
    // (first fit of this workspace) all three.  The kernels themselves decide which of the launched ones runs, from
    // THIS fit's depth (fit_hist_runs) -- no host round trip, and a stale hint costs time, never correctness.
    const int launched = fitjob::launched_geometries(j.hist, *(volatile int*)w.h_depth.get());
    HIP_TRY(hipMemcpyAsync(w.h_depth, w.depth, 4, hipMemcpyDeviceToHost, st));
    const FitHistArgs a{j, st, w.hs.hist, w.hs.ov_y, w.hs.ov_r, w.hs.ovn, w.cap, w.eta, w.lam, w.done, w.depth, w.fevals, launched};
    auto each_geometry = [&](auto step) { step(hg8::Launch()); step(hg4::Launch()); step(hg2::Launch()); };
    each_geometry([&](auto g) { if (g.on(a)) g.hist(a); });
    if (j.mode == 1) each_geometry([&](auto g) { if (g.on(a)) g.nm(a); });
    else each_geometry([&](auto g) { if (g.on(a)) g.newton(a); });
    HIP_TRY(hipGetLastError());
    return ED_OK;
  }
  const int64_t tmod = j.tmod;
  const bool skips = j.skip_K > 0 && tmod > 0 && j.d_skip_from;
  if (skips)
    hipLaunchKernelGGL(k_fit_skip_prefixes, dim3((unsigned)((tmod + 255) / 256)), dim3(256), 0, st, w.eta, w.done, j.skip_K, tmod, 0.04, j.d_skip_from);
  // coarse Newton steps on every 16th exon, then full passes until the step is below tolerance
  const int coarse = (E >= 8192) ? kFitCoarsePasses : 0;   // a stride-16 subset below ~500 exons is too noisy to help
  const int cstride = 16;                   // (8 / 4 / 2 measured on the cohort reference sets' 10 000-row fit: 9.9 / 11.1 / 12.3 ms against 9.6)
  // Prefixes closed before the first pass (k_fit_skip_prefixes) are lanes that idle through every pass: the columns that iterate are packed from the
  // start then (round 6), and again before each of the first full passes as columns converge.  Which slot a column takes does not show in its sums:
  // k_fit_accum picks its digamma series per lane, and k_fit_update reduces a slot's partials in chunk order (tests/test_gpu_fit_invariance.py).
  const bool can_pack = S >= 4096 && w.colmap;
  const bool pack_early = can_pack && skips;
  auto compact = [&]() {
    (void)hipMemsetAsync(w.n_map, 0, 4, st);
    hipLaunchKernelGGL(k_fit_compact, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, w.done, S, w.colmap, w.n_map);
  };
  if (pack_early) compact();
  for (int it = 0; it < coarse; ++it) {
    hipLaunchKernelGGL(k_fit_accum, grid, block, 0, st, j.test, j.trs, j.tcs, j.ref, j.rrs, E, S, cstride, w.eta, w.lam, w.done, w.partial, tmod,
                       pack_early ? w.colmap : (const int32_t*)nullptr, pack_early ? w.n_map : (const int*)nullptr);
    hipLaunchKernelGGL(k_fit_update, gr, br, 0, st, w.partial, nch, S, w.eta, w.lam, w.done, 1e-6, 0,
                       pack_early ? w.colmap : (const int32_t*)nullptr, pack_early ? w.n_map : (const int*)nullptr);
  }
  // (round 5: two passes on every 4th exon between the coarse and the full ones were tried -- 9.2 -> 10.0 ms for the cohort reference sets'
  //  32 768 columns: the full passes needed are the same three, the medium ones came on top)
  // The looser stopping rule is the reference-set searches' (one test column shared by the columns, or the test columns taken cyclically), whose fits feed a
  // choice among candidates; a fit handed back as the sample's (phi, expected) keeps 1e-6 -- on a column with phi ~ 8e-6 the constant C of the header above is
  // ~500 and 2e-5 left 1.9e-7 (tests/test_gpu_fit.py::test_per_cell_fit_on_ill_conditioned_columns; ADVICE r5).
  const double step_tol = (j.view == FitJob::kSharedTest || j.view == FitJob::kCyclicTest) ? kFitStepTol : 1e-6;
  for (int it = 0; it < 10; ++it) {   // converged columns skip their work; typically 3 passes do something
    // from the fourth pass on: the columns still iterating packed into the first waves (k_fit_compact), many columns only
    const bool packed = can_pack && (it >= 3 || pack_early);
    if (packed && (it == 3 || (pack_early && it >= 1 && it < 3))) compact();
    hipLaunchKernelGGL(k_fit_accum, grid, block, 0, st, j.test, j.trs, j.tcs, j.ref, j.rrs, E, S, 1, w.eta, w.lam, w.done, w.partial, tmod,
                       packed ? w.colmap : (const int32_t*)nullptr, packed ? w.n_map : (const int*)nullptr);
    hipLaunchKernelGGL(k_fit_update, gr, br, 0, st, w.partial, nch, S, w.eta, w.lam, w.done, step_tol, 1,
                       packed ? w.colmap : (const int32_t*)nullptr, packed ? w.n_map : (const int*)nullptr);
  }
  hipLaunchKernelGGL(k_fit_finish, g1, b1, 0, st, w.eta, w.lam, S, j.phi, j.expected);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}
