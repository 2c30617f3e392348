// edbins_hist.inc -- the depth-binned dispersion fit (phi.bins > 1, R/class_definition.R:120-147) on COUNT HISTOGRAMS.
// Included by edbins.inc inside its anonymous namespace.  Round 2's form of this fit walked the count matrix 17 times for the
// 0.85 quantile of the reference counts (bisection on the value) and 6+ times for the Newton iteration on (eta, lambda_1..B):
// 17.5 ms at 200 000 x 1024 next to 1.4 ms for the single-dispersion fit.  Every term of the grouped likelihood still depends
// on ONE count and on the level of the cell, and the level (depth.quant = cut(reference, complete.bins)) is a function of the
// reference count alone, so three passes over the counts are enough:
//   k_lh_rhist   reference counts only: unit bins r < 8192 of every column (+ column maximum, + how many lie beyond)
//   k_lh_select  the two order statistics of quantile(reference, 0.85) read off the cumulative histogram     -> k_bins_edges
//   k_lh_hist    per LEVEL: unit bins of the test count (y < 1024) and of the total shifted by the level's smallest reference
//                count (n - lo_g < 4096); a cell with a count outside its bins goes to a list (row order, no atomics)
//   k_lh_lists   the lists of a sample merged into one array sorted by level (once per fit) + the population of every level
//   k_lh_newton  all Newton passes in one launch; a pass = sums over (B x 5120 + 8192) bins and the listed cells, per level, then the
//                step of edbins.inc's fitb_step (the function the per-cell form's k_fitb_update calls)
// The sums are formed from differences psi(shape + v) - psi(shape) along blocks of consecutive bins, as k_fit_hnewton does
// (edfit_hist.inc); the terms of a cell are covered one by one: its y term by the level's y bins or the list, its n term by the
// level's n bins or the list, its r term by the column's r bins or the list.
// Anything this form cannot hold (a quantile beyond the r bins, a list that ran out, a count >= 2^28) raises a device flag and
// the caller runs the per-cell form of edbins.inc instead -- same answer to the fit's tolerance.

constexpr int kLhKq = 8192;                  // unit bins of the reference count
constexpr int kLhQS = 8;                     // samples per workgroup of k_lh_rhist (8 x 8192 16-bit bins = 128 KB of LDS)
constexpr int kLhKy = 1024, kLhKn = 4096;    // per level: bins of the test count and of the shifted total
constexpr int kLhK = kLhKy + kLhKn;
constexpr int kLhBlock = 1024;
constexpr int kLhHalves = 2;                 // workgroups per sample group: each takes half of the rows
constexpr int kLhChunk = 65535;              // rows between flushes: a 16-bit LDS bin cannot wrap
constexpr int kLhListTotal = 32768;          // listed cells per sample: regions x cap, and the size of the sorted array
constexpr int kLhS = 4, kLhY = 256;          // k_lh_lists / k_lh_accum: samples per workgroup, strands per sample
enum { LH_FLAG_QUANTILE = 1, LH_FLAG_LIST = 2, LH_FLAG_RANGE = 4 };

__host__ __device__ __forceinline__ int64_t lh_padded(int64_t S) { return (S + 7) / 8 * 8; }
// [half][quad of samples][bin][4]: a wave of k_lh_accum (4 samples x 16 strands) reads contiguous runs, the flushes write whole lines
__device__ __forceinline__ int64_t lh_at(int half, int64_t K, int64_t v, int64_t s, int64_t Sp)
{
  return (((int64_t)half * (Sp >> 2) + (s >> 2)) * K + v) * 4 + (s & 3);
}

// which (half, sample group) this workgroup serves: XCD x (= blockIdx % 8) owns a contiguous range of the pairs, so that
// the workgroups sharing the 128-byte lines of a count row sit behind one L2 (as k_fit_hist)
__device__ __forceinline__ bool lh_place(int64_t ng, int& half, int64_t& grp)
{
  const int64_t nwg = ng * kLhHalves, per = (nwg + 7) / 8;
  const int64_t lin = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const bool active = (int64_t)(blockIdx.x >> 3) < per && lin < nwg;
  half = active ? (int)(lin / ng) : 0;
  grp = active ? lin % ng : 0;
  return active;
}
static inline unsigned lh_grid(int64_t ng) { return (unsigned)(((ng * kLhHalves + 7) / 8) * 8); }

__global__ void __launch_bounds__(kLhBlock)
k_lh_rhist(const int32_t* __restrict__ ref, int64_t E, int64_t S, uint32_t* __restrict__ hist, int32_t* __restrict__ xmax,
           uint32_t* __restrict__ beyond)
{
  __shared__ uint32_t hsm[kLhQS * (kLhKq / 2)];
  __shared__ int sh_max[kLhQS];
  __shared__ uint32_t sh_bey[kLhQS];
  const int tid = threadIdx.x;
  int half; int64_t grp;
  const bool active = lh_place((S + kLhQS - 1) / kLhQS, half, grp);
  constexpr int kRows = kLhBlock / kLhQS;
  const int j = tid & (kLhQS - 1);
  const int64_t s = active ? grp * kLhQS + j : S;
  uint32_t* __restrict__ h = hsm + j * (kLhKq / 2);
  const int64_t Sp = lh_padded(S);
  const int64_t r0 = (E * half) / kLhHalves, r1 = (E * (half + 1)) / kLhHalves;
  if (tid < kLhQS) { sh_max[tid] = 0; sh_bey[tid] = 0u; }
  int m = 0; uint32_t bey = 0;
  int chunk_no = 0;
  for (int64_t c0 = r0; c0 < r1 || chunk_no == 0; c0 += kLhChunk, ++chunk_no) {
    const int64_t c1 = (c0 + kLhChunk < r1) ? c0 + kLhChunk : r1;
    for (int i = tid; i < kLhQS * (kLhKq / 2); i += kLhBlock) hsm[i] = 0;
    __syncthreads();
    if (s < S) {
      constexpr int kPre = 8;
      for (int64_t e = c0 + tid / kLhQS; e < c1; e += (int64_t)kPre * kRows) {
        int rb[kPre];
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          const int64_t en = e + (int64_t)k * kRows;
          rb[k] = (en < c1) ? ref[en * S + s] : -1;
        }
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          if (e + (int64_t)k * kRows >= c1) break;
          const int r = rb[k];
          m = max(m, r);
          if ((unsigned)r < (unsigned)kLhKq) atomicAdd(&h[r >> 1], 1u << ((r & 1) * 16));
          else ++bey;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < kLhQS * kLhKq; i += kLhBlock) {
      const int quad = i / (kLhKq * 4), rem = i % (kLhKq * 4);
      const int v = rem >> 2, jj = quad * 4 + (rem & 3);
      const int64_t ss = grp * kLhQS + jj;
      if (active && ss < S) {
        const uint32_t cnt = (hsm[jj * (kLhKq / 2) + (v >> 1)] >> ((v & 1) * 16)) & 0xffffu;
        uint32_t* __restrict__ o = hist + lh_at(half, kLhKq, v, ss, Sp);
        *o = (chunk_no == 0 ? 0u : *o) + cnt;
      }
    }
    __syncthreads();
  }
  if (s < S) { atomicMax(&sh_max[j], m); atomicAdd(&sh_bey[j], bey); }
  __syncthreads();
  if (tid < kLhQS && active && grp * kLhQS + tid < S) {
    atomicMax(&xmax[grp * kLhQS + tid], sh_max[tid]);
    atomicAdd(&beyond[grp * kLhQS + tid], sh_bey[tid]);
  }
}

// order statistics k0 <= k1 (0-based ranks) of every column's reference counts from the cumulative r histogram
__global__ void __launch_bounds__(kLhS * kLhY)
k_lh_select(const uint32_t* __restrict__ hist, int64_t S, int64_t k0, int64_t k1, int32_t* __restrict__ x0, int32_t* __restrict__ x1,
            int* __restrict__ flags)
{
  __shared__ uint32_t c[kLhKq][kLhS];
  __shared__ uint32_t pre[kLhY + 1][kLhS];
  const int lane = threadIdx.x, y = threadIdx.y;
  const int64_t s = (int64_t)blockIdx.x * kLhS + lane;
  const bool live = s < S;
  const int64_t sc = live ? s : S - 1, Sp = lh_padded(S);
  for (int v = y; v < kLhKq; v += kLhY) c[v][lane] = hist[lh_at(0, kLhKq, v, sc, Sp)] + hist[lh_at(1, kLhKq, v, sc, Sp)];
  __syncthreads();
  constexpr int nb = kLhKq / kLhY;
  uint32_t sum = 0;
  for (int i = 0; i < nb; ++i) sum += c[y * nb + i][lane];
  pre[y + 1][lane] = sum;
  __syncthreads();
  if (y == 0) {
    uint32_t run = 0;
    pre[0][lane] = 0;
    for (int i = 1; i <= kLhY; ++i) { run += pre[i][lane]; pre[i][lane] = run; }
  }
  __syncthreads();
  if (!live) return;
  // (a rank beyond the bins leaves 0 in both and raises the flag: the caller discards this form's results)
  if (y == kLhY - 1 && k1 >= (int64_t)pre[kLhY][lane]) {
    atomicOr(flags, (int)LH_FLAG_QUANTILE);
    if (k0 >= (int64_t)pre[kLhY][lane]) x0[s] = 0;
    x1[s] = 0;
  }
  const int64_t before = pre[y][lane];
  for (int w = 0; w < 2; ++w) {
    const int64_t k = w ? k1 : k0;
    if (before <= k && k < before + (int64_t)sum) {
      int64_t cum = before;
      for (int i = 0; i < nb; ++i) {
        cum += c[y * nb + i][lane];
        if (cum > k) { (w ? x1 : x0)[s] = y * nb + i; break; }
      }
    }
  }
}

// smallest reference count of every level (lo[0] = 0; lo[k >= B] = INT_MAX): r is in level g  <=>  lo[g] <= r < lo[g + 1]
// (bins_group counts the edges <= r; r an integer, so r >= edge  <=>  r >= ceil(edge))
__device__ __forceinline__ void lh_level_bounds(const double* __restrict__ edges, int B, int64_t S, int64_t s, int (&lo)[kMaxPhiBins])
{
#pragma unroll
  for (int k = 0; k < kMaxPhiBins; ++k) {
    double e = (k < B) ? edges[(int64_t)k * S + s] : 4e9;
    e = ceil(e);
    lo[k] = (k == 0) ? 0 : ((e < 2147483647.0) ? (int)e : 2147483647);
  }
}

// per-level unit bins of the test count and of the shifted total; KS samples per workgroup share the LDS
// (B x 5120 16-bit bins each: KS = 4 up to B = 3, 2 up to B = 7, 1 at B = 8)
template <int KS>
__global__ void __launch_bounds__(kLhBlock)
k_lh_hist(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t E, int64_t S, int B,
          const double* __restrict__ edges, uint32_t* __restrict__ hist, int32_t* __restrict__ ov_y, int32_t* __restrict__ ov_r,
          int32_t* __restrict__ ovn, int cap, int* __restrict__ flags)
{
  extern __shared__ uint32_t lsm[];
  if (*flags & LH_FLAG_QUANTILE) return;   // the edges mean nothing: this form has already declined
  const int tid = threadIdx.x;
  int half; int64_t grp;
  const bool active = lh_place((S + KS - 1) / KS, half, grp);
  constexpr int kRows = kLhBlock / KS;
  const int j = tid & (KS - 1);
  const int64_t s = active ? grp * KS + j : S;
  const int KB = B * kLhK, W = KB / 2;
  uint32_t* __restrict__ h = lsm + j * W;
  const int64_t Sp = lh_padded(S);
  const int64_t r0 = (E * half) / kLhHalves, r1 = (E * (half + 1)) / kLhHalves;
  int lo[kMaxPhiBins];
  lh_level_bounds(edges, B, S, s < S ? s : S - 1, lo);
  int nov = 0;
  const int region = half * kRows + tid / KS;
  const int64_t ovbase = (int64_t)region * cap;
  bool bad = false;
  int chunk_no = 0;
  for (int64_t c0 = r0; c0 < r1 || chunk_no == 0; c0 += kLhChunk, ++chunk_no) {
    const int64_t c1 = (c0 + kLhChunk < r1) ? c0 + kLhChunk : r1;
    for (int i = tid; i < KS * W; i += kLhBlock) lsm[i] = 0;
    __syncthreads();
    if (s < S) {
      constexpr int kPre = 4;
      for (int64_t e = c0 + tid / KS; e < c1; e += (int64_t)kPre * kRows) {
        int yb[kPre], rb[kPre];
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          const int64_t en = e + (int64_t)k * kRows;
          yb[k] = (en < c1) ? test[en * S + s] : 0;
          rb[k] = (en < c1) ? ref[en * S + s] : 0;
        }
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          if (e + (int64_t)k * kRows >= c1) break;
          const int y = yb[k], r = rb[k];
          const int n = y + r;
          if (n <= 0) continue;   // psi(x + 0) - psi(x) = 0 in every term
          int g = 0, lg = 0;
#pragma unroll
          for (int q = 1; q < kMaxPhiBins; ++q) { const bool in = r >= lo[q]; g += in ? 1 : 0; lg = in ? lo[q] : lg; }
          const bool oy = (unsigned)y >= (unsigned)kLhKy, on = (unsigned)(n - lg) >= (unsigned)kLhKn, orr = (unsigned)r >= (unsigned)kLhKq;
          if (!oy) { const int v = g * kLhK + y; atomicAdd(&h[v >> 1], 1u << ((v & 1) * 16)); }
          if (!on) { const int v = g * kLhK + kLhKy + (n - lg); atomicAdd(&h[v >> 1], 1u << ((v & 1) * 16)); }
          if (oy || on || orr) {
            if ((unsigned)y >= (1u << 28)) bad = true;
            if (nov < cap) { ov_y[(ovbase + nov) * S + s] = (y & 0x0fffffff) | (g << 28); ov_r[(ovbase + nov) * S + s] = r; }
            ++nov;
          }
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < KS * KB; i += kLhBlock) {
      const int v = i / KS, jj = i % KS;
      const int64_t ss = grp * KS + jj;
      if (active && ss < S) {
        const uint32_t cnt = (lsm[jj * W + (v >> 1)] >> ((v & 1) * 16)) & 0xffffu;
        uint32_t* __restrict__ o = hist + lh_at(half, KB, v, ss, Sp);
        *o = (chunk_no == 0 ? 0u : *o) + cnt;
      }
    }
    __syncthreads();
  }
  if (s < S) {
    ovn[(int64_t)region * S + s] = nov;
    if (nov > cap) atomicOr(flags, (int)LH_FLAG_LIST);
    if (bad) atomicOr(flags, (int)LH_FLAG_RANGE);
  }
}

// The lists of a sample (nreg regions, row order inside each) merged into one array ordered by level, and the population of
// every level (all exons: R/class_definition.R:130-133) from the r histogram.  Strand y owns regions y, y + 256, ...
__global__ void __launch_bounds__(kLhS * kLhY)
k_lh_lists(const int32_t* __restrict__ ov_y, const int32_t* __restrict__ ov_r, const int32_t* __restrict__ ovn, int cap, int nreg,
           int64_t S, int B, const double* __restrict__ edges, const uint32_t* __restrict__ rhist, const uint32_t* __restrict__ beyond,
           int2* __restrict__ sorted, int* __restrict__ lvl_start, double* __restrict__ pop, int* __restrict__ flags)
{
  if (*flags & LH_FLAG_QUANTILE) return;
  __shared__ int cnt[kLhS][kMaxPhiBins][kLhY];
  __shared__ int start[kLhS][kMaxPhiBins + 1];
  __shared__ uint32_t sh_pop[kLhS][kMaxPhiBins];
  const int lane = threadIdx.x, y = threadIdx.y;
  const int64_t s = (int64_t)blockIdx.x * kLhS + lane;
  const bool live = s < S;
  const int64_t sc = live ? s : S - 1, Sp = lh_padded(S);
  for (int g = 0; g < kMaxPhiBins; ++g) cnt[lane][g][y] = 0;
  if (y < kMaxPhiBins) sh_pop[lane][y] = 0u;
  __syncthreads();
  for (int reg = y; reg < nreg; reg += kLhY) {
    const int c = min(ovn[(int64_t)reg * S + sc], cap);
    for (int i = 0; i < c; ++i) {
      const int g = (int)((uint32_t)ov_y[((int64_t)reg * cap + i) * S + sc] >> 28);
      cnt[lane][g][y] += 1;
    }
  }
  __syncthreads();
  if (y < B) {                       // one strand per level: exclusive prefix over the strands
    int run = 0;
    for (int i = 0; i < kLhY; ++i) { const int t = cnt[lane][y][i]; cnt[lane][y][i] = run; run += t; }
    start[lane][y + 1] = run;        // the level's total for now
  }
  __syncthreads();
  if (y == 0) {
    int run = 0;
    start[lane][0] = 0;
    for (int g = 1; g <= B; ++g) { run += start[lane][g]; start[lane][g] = run; }
    if (run > kLhListTotal) atomicOr(flags, (int)LH_FLAG_LIST);
    if (live) for (int g = 0; g <= B; ++g) lvl_start[(int64_t)g * S + s] = min(start[lane][g], kLhListTotal);
  }
  __syncthreads();
  for (int reg = y; reg < nreg; reg += kLhY) {
    const int c = min(ovn[(int64_t)reg * S + sc], cap);
    for (int i = 0; i < c; ++i) {
      const int yy = ov_y[((int64_t)reg * cap + i) * S + sc], rr = ov_r[((int64_t)reg * cap + i) * S + sc];
      const int g = (int)((uint32_t)yy >> 28);
      const int at = start[lane][g] + cnt[lane][g][y];
      cnt[lane][g][y] += 1;
      if (live && at < kLhListTotal) sorted[sc * kLhListTotal + at] = make_int2(yy & 0x0fffffff, rr);
    }
  }
  // population of the levels
  int lo[kMaxPhiBins];
  lh_level_bounds(edges, B, S, sc, lo);
  constexpr int nb = kLhKq / kLhY;
  for (int i = 0; i < nb; ++i) {
    const int v = y * nb + i;
    const uint32_t c = rhist[lh_at(0, kLhKq, v, sc, Sp)] + rhist[lh_at(1, kLhKq, v, sc, Sp)];
    int g = 0;
#pragma unroll
    for (int q = 1; q < kMaxPhiBins; ++q) g += (v >= lo[q]) ? 1 : 0;
    if (c) atomicAdd(&sh_pop[lane][g], c);
  }
  __syncthreads();
  if (live && y < B) {
    // counts beyond the r bins lie above the 0.85 quantile (k_lh_select found it inside the bins): the last level
    pop[(int64_t)y * S + s] = (double)sh_pop[lane][y] + ((y == B - 1) ? (double)beyond[s] : 0.0);
  }
}

// sum over a run of consecutive bins of count x (psi(x + k) - psi(x0), psi'(x + k) - psi'(x0)), k = 0..nb-1: hn_block of
// edfit_hist.inc for runs of any length, counts = the two halves of a global histogram (one bin every 4 words)
__device__ __noinline__ double2 lh_block(double x, int nb, const uint32_t* __restrict__ g0, const uint32_t* __restrict__ g1,
                                         double ix0, double r0, double q0)
{
  double x1, r1, q1;
  edfit::digamma_trigamma_nolog(x, x1, r1, q1);
  double dh = edfit::flog(x1 * ix0) + (r1 - r0), dl = 0.0;
  double dq = q1 - q0;
  double g = 0.0, h = 0.0;
  constexpr int kChunk = 4;
  for (int k0 = 0; k0 < nb; k0 += kChunk) {
    uint32_t c[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const int k = k0 + j;
      c[j] = (k < nb) ? g0[4 * k] + g1[4 * k] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const double cd = (double)c[j];
      g = __builtin_fma(cd, dh + dl, g);
      h = __builtin_fma(cd, dq, h);
      const double r = edfit::frcp(x + (double)(k0 + j));
      const double t = dh + r;
      const double bb = t - dh;
      dl += (dh - (t - bb)) + (r - bb);
      dh = t;
      dq = __builtin_fma(-r, r, dq);
    }
  }
  return make_double2(g, h);
}

// The Newton iteration of 4 samples in one launch: per pass the gradient / Hessian sums of every level -- over the level's y and n
// bins, its run of the column's r bins and its listed cells -- added up in a fixed-order LDS tree, then strand 0 of each sample takes
// the step (fitb_step of edbins.inc: the very function k_fitb_update calls in the per-cell form) and publishes the new point through
// LDS.  partial[6 g + (ga, gb, haa, hab, hbb, 0)][S] is the scratch the sums go through (the constant terms are inside the differences:
// the cell count is 0).
__device__ __noinline__ void fitb_step(const double (*tot)[6], int B, int64_t S, int64_t s, double* __restrict__ eta,
                                       double* __restrict__ lam, double* __restrict__ state, int* __restrict__ done, double tol,
                                       int final_pass);

__global__ void __launch_bounds__(kLhS * kLhY)
k_lh_newton(const uint32_t* __restrict__ lhist, const uint32_t* __restrict__ rhist, const int2* __restrict__ sorted,
            const int* __restrict__ lvl_start, int64_t S, int B, const double* __restrict__ edges, double* __restrict__ eta,
            double* __restrict__ lam, int* __restrict__ done, double* __restrict__ partial, const int* __restrict__ flags,
            double* __restrict__ state, int max_iter, double tol)
{
  if (*flags) return;   // this form has declined (the caller runs the per-cell form): nothing here is used
  __shared__ double lds[5][kLhY][kLhS];
  __shared__ double sh_eta[kLhS], sh_lam[kMaxPhiBins][kLhS];
  __shared__ int sh_done[kLhS];
  const int lane = threadIdx.x, y = threadIdx.y;
  const int64_t s = (int64_t)blockIdx.x * kLhS + lane;
  const bool live = s < S;
  const int64_t sc = live ? s : S - 1, Sp = lh_padded(S);
  if (y == 0) {
    sh_eta[lane] = eta[sc];
    for (int g = 0; g < B; ++g) sh_lam[g][lane] = lam[(int64_t)g * S + sc];
    sh_done[lane] = live ? done[sc] : 1;
  }
  int lo[kMaxPhiBins];
  lh_level_bounds(edges, B, S, sc, lo);
  const int KB = B * kLhK;
  __syncthreads();
  for (int it = 0; it < max_iter; ++it) {
    const int dn = sh_done[lane];
    if (__syncthreads_and(dn)) break;
    const double p = 1.0 / (1.0 + ed_pexp(-sh_eta[lane]));
    for (int g = 0; g < B; ++g) {
      double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (!dn) {
        const double th = ed_pexp(sh_lam[g][lane]);
        const double a = th * p, b = th * (1.0 - p);
        double xa, ra, qa, xb, rb, qb, xt, rt, qt;
        edfit::digamma_trigamma_nolog(a, xa, ra, qa);
        edfit::digamma_trigamma_nolog(b, xb, rb, qb);
        edfit::digamma_trigamma_nolog(th, xt, rt, qt);
        const double ixa = edfit::frcp(xa), ixb = edfit::frcp(xb), ixt = edfit::frcp(xt);
        int lg = 0, hg = 2147483647;
#pragma unroll
        for (int q = 1; q < kMaxPhiBins; ++q) { lg = (q == g) ? lo[q] : lg; hg = (q == g + 1) ? lo[q] : hg; }
        {
          constexpr int nb = kLhKy / kLhY;
          const int v = g * kLhK + y * nb;
          const double2 t = lh_block(a + (double)(y * nb), nb, lhist + lh_at(0, KB, v, sc, Sp), lhist + lh_at(1, KB, v, sc, Sp), ixa, ra, qa);
          acc[0] += t.x; acc[2] += t.y;
        }
        {
          constexpr int nb = kLhKn / kLhY;
          const int v = g * kLhK + kLhKy + y * nb;
          const double2 t = lh_block(th + (double)lg + (double)(y * nb), nb, lhist + lh_at(0, KB, v, sc, Sp), lhist + lh_at(1, KB, v, sc, Sp),
                                     ixt, rt, qt);
          acc[0] -= t.x; acc[1] -= t.x;
          acc[2] -= t.y; acc[3] -= t.y; acc[4] -= t.y;
        }
        {
          constexpr int nb = kLhKq / kLhY;
          const int v0 = max(y * nb, lg), v1 = min(y * nb + nb, hg);
          if (v0 < v1) {
            const double2 t = lh_block(b + (double)v0, v1 - v0, rhist + lh_at(0, kLhKq, v0, sc, Sp), rhist + lh_at(1, kLhKq, v0, sc, Sp),
                                       ixb, rb, qb);
            acc[1] += t.x; acc[4] += t.y;
          }
        }
        const int q0 = lvl_start[(int64_t)g * S + sc], q1 = lvl_start[(int64_t)(g + 1) * S + sc];
        for (int q = q0 + y; q < q1; q += kLhY) {
          const int2 cell = sorted[sc * kLhListTotal + q];
          const int yy = cell.x, rr = cell.y, nn = yy + rr;
          double x1, r1, q1v;
          if (yy >= kLhKy) {
            edfit::digamma_trigamma_nolog(a + (double)yy, x1, r1, q1v);
            acc[0] += edfit::flog(x1 * ixa) + (r1 - ra); acc[2] += q1v - qa;
          }
          if (rr >= kLhKq) {
            edfit::digamma_trigamma_nolog(b + (double)rr, x1, r1, q1v);
            acc[1] += edfit::flog(x1 * ixb) + (r1 - rb); acc[4] += q1v - qb;
          }
          if (nn - lg >= kLhKn) {
            edfit::digamma_trigamma_nolog(th + (double)nn, x1, r1, q1v);
            const double t = edfit::flog(x1 * ixt) + (r1 - rt), tq = q1v - qt;
            acc[0] -= t; acc[1] -= t;
            acc[2] -= tq; acc[3] -= tq; acc[4] -= tq;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) lds[q][y][lane] = acc[q];
      __syncthreads();
      for (int hh = kLhY / 2; hh >= 1; hh >>= 1) {
        if (y < hh) {
#pragma unroll
          for (int q = 0; q < 5; ++q) lds[q][y][lane] += lds[q][y + hh][lane];
        }
        __syncthreads();
      }
      if (y == 0 && live && !dn) {
#pragma unroll
        for (int q = 0; q < 5; ++q) partial[(int64_t)(g * 6 + q) * S + s] = lds[q][0][lane];
        partial[(int64_t)(g * 6 + 5) * S + s] = 0.0;
      }
      __syncthreads();
    }
    if (y == 0 && live && !dn) {
      double tot[kMaxPhiBins][6];
      for (int g = 0; g < B; ++g)
        for (int q = 0; q < 6; ++q) tot[g][q] = partial[(int64_t)(g * 6 + q) * S + s];   // (this thread's own stores)
      fitb_step(tot, B, S, s, eta, lam, state, done, tol, 1);
      sh_eta[lane] = eta[s];
      for (int g = 0; g < B; ++g) sh_lam[g][lane] = lam[(int64_t)g * S + s];
      sh_done[lane] = done[s];
    }
    __syncthreads();
  }
}

// device buffers of the histogram form, kept on the batch (hipFree would synchronise the device on every fit)
struct BinsWork {
  int64_t E = 0, S = 0; int B = 0;
  DevBuf<uint32_t> rhist, lhist, beyond;
  DevBuf<int32_t> xmax, x0, x1, ov_y, ov_r, ovn;
  DevBuf<int2> sorted;
  DevBuf<int> lvl_start, flags, done;
  DevBuf<double> pop, eta, lam, state, part;
  PinBuf<void> host;   // pinned: flags (1 int), done (S ints), pop (kMaxPhiBins x S doubles)
  Event ev;            // the three copies into `host` of the last fit are complete
  int alloc(int64_t E_, int64_t S_, int B_)
  {
    if (E_ == E && S_ == S && B_ <= B) return ED_OK;
    *this = BinsWork();
    const int64_t Sp = lh_padded(S_);
    HIP_TRY(rhist.alloc((size_t)kLhHalves * Sp * kLhKq * 4));
    HIP_TRY(lhist.alloc((size_t)kLhHalves * Sp * B_ * kLhK * 4));
    HIP_TRY(beyond.alloc((size_t)S_ * 4));
    HIP_TRY(xmax.alloc((size_t)S_ * 4));
    HIP_TRY(x0.alloc((size_t)S_ * 4));
    HIP_TRY(x1.alloc((size_t)S_ * 4));
    HIP_TRY(ov_y.alloc((size_t)kLhListTotal * S_ * 4));
    HIP_TRY(ov_r.alloc((size_t)kLhListTotal * S_ * 4));
    HIP_TRY(ovn.alloc((size_t)(kLhHalves * kLhBlock) * S_ * 4));
    HIP_TRY(sorted.alloc((size_t)kLhListTotal * S_ * 8));
    HIP_TRY(lvl_start.alloc((size_t)(kMaxPhiBins + 1) * S_ * 4));
    HIP_TRY(flags.alloc(4));
    HIP_TRY(done.alloc((size_t)S_ * 4));
    HIP_TRY(pop.alloc((size_t)kMaxPhiBins * S_ * 8));
    HIP_TRY(eta.alloc((size_t)S_ * 8));
    HIP_TRY(lam.alloc((size_t)kMaxPhiBins * S_ * 8));
    HIP_TRY(state.alloc((size_t)(2 * (kMaxPhiBins + 1) + 2) * S_ * 8));
    HIP_TRY(part.alloc((size_t)6 * kMaxPhiBins * S_ * 8));
    HIP_TRY(host.alloc(4 + (size_t)S_ * 4 + 4 + (size_t)kMaxPhiBins * S_ * 8));
    HIP_TRY(ev.create(hipEventDisableTiming));
    E = E_; S = S_; B = B_;
    return ED_OK;
  }
};
