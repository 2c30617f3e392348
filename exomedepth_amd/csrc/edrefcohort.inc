// edrefcohort.inc -- select.reference.set for EVERY sample of a cohort at once (included at the end of edcore.hip).
//
// The reference's canonical workflow (vignette/vignette.Rnw:390-431) runs, for each test sample, select.reference.set against
// all other samples of the cohort (R/optimize_reference_set.R:53-148) and sums the chosen references into the aggregate
// reference the model is then fitted against (vignette.Rnw:393-402).  Done one test sample at a time that is S calls of
// ed_select_reference_set -- tens of seconds for S = 1024 next to a 10 ms emission / Viterbi step.  Here, for all S tests:
//   :79-88   the bin selection depends on rowSums(reference.counts) + test.counts = the row sums over ALL samples: shared by every test
//   :100     the correlations of the length/depth-normalised counts between every pair of samples: ONE S x S Gram matrix of the
//            centred normalised count matrix Z [n_bins_selected][S] in binary64 -- the one dense contraction on this path, done
//            with v_mfma_f64_16x16x4_f64 (k_rc_gram).  2 n S^2 flop: 2e10 at n = 10 000, S = 1024 -- 0.3 ms at the FP64 matrix
//            peak, so the kernel is bound by reading Z (80 MB) and is launch-latency sized; it is here because it is the right
//            instruction for the shape, not because it moves the needle
//   :101-102 per test the other samples in order of decreasing correlation (host: S sorts of S - 1 values)
//   :114-141 the loop over cumulative references stops at the first i > 2 with mean.p < 0.05 (:130): only the first K prefixes
//            (K = max_refs, default 32) are formed and fitted -- as ONE batched fit of K x T columns per chunk of T tests
//            (fit_columns with the test column taken modulo T) -- and a test whose loop would run beyond K falls back to
//            ed_select_reference_set, so the answer never depends on K
//   :143-145 the choice; then the aggregate reference of every sample, for all exons, on the device (k_rc_aggregate): the
//            ref[E][S] matrix ed_batch_run / ed_cohort_submit consume
// Parity: the same tolerance-level statement as edrefset.inc (aod / VGAM are not in the reference tree); against S independent
// ed_select_reference_set calls: identical choices, statistics to rounding (tests/test_gpu_refcohort.py).

namespace {

// compact the selected bins: X[e][s] = counts[sel[e]][s]
__global__ void __launch_bounds__(256)
k_rc_compact(const int32_t* __restrict__ counts, const int32_t* __restrict__ sel, int64_t n, int64_t S, int32_t* __restrict__ X)
{
  const int64_t e = blockIdx.y;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n && s < S) X[e * S + s] = counts[(int64_t)sel[e] * S + s];
}

// Z[e][s] = u - mean_s,  u = x / (len * colsum_s / 1e6)   (R/optimize_reference_set.R:100; rs_norm), rows padded to a multiple of 4
__global__ void __launch_bounds__(256)
k_rc_centre(const int32_t* __restrict__ X, const int32_t* __restrict__ sel, const double* __restrict__ len, int64_t n, int64_t S,
            const double* __restrict__ colsum, const double* __restrict__ colmean, int64_t Sp, double* __restrict__ Z)
{
  const int64_t e = blockIdx.y;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= Sp) return;
  double z = 0.0;
  if (e < n && s < S) {
    const double L = len ? len[sel[e]] : 1.0;
    z = rs_norm((double)X[e * S + s], L, colsum[s]) - colmean[s];
  }
  Z[e * Sp + s] = z;
}

// G = Z^T Z (S x S, binary64) with v_mfma_f64_16x16x4_f64: a wave owns a 32 x 32 block of G (2 x 2 MFMA tiles, so every
// A / B fragment loaded feeds two instructions) and walks a SLICE of the rows of Z four at a time; the slices' partial blocks
// are added in a fixed order by k_rc_gram_sum (no floating-point atomics: the correlations, hence the order of near-tied
// references, are the same on every run).  Fragment layout (cdna_hip_programming.md): A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15], one f64 per lane; D: col = lane & 15, row = (lane >> 4) + 4 * reg.
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int kGramSlices = 16;
__global__ void __launch_bounds__(64)
k_rc_gram(const double* __restrict__ Z, int64_t n4 /* rows, multiple of 4 */, int64_t Sp /* multiple of 32 */, double* __restrict__ part /* [slices][Sp][Sp] */,
          int64_t blk_lo, int64_t blk_hi /* only blocks with a row or column block in [blk_lo, blk_hi), and the diagonal blocks */)
{
  const int lane = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * 32, b0 = (int64_t)blockIdx.y * 32;
  if (b0 > a0) return;                                   // G is symmetric: the lower triangle of blocks; k_rc_gram_sum mirrors
  {
    const int64_t ba = blockIdx.x, bb = blockIdx.y;      // a test range [tb, te) needs rows tb..te-1 of G and its diagonal only
    if (!((ba >= blk_lo && ba < blk_hi) || (bb >= blk_lo && bb < blk_hi) || ba == bb)) return;
  }
  const int64_t steps = n4 / 4, per = (steps + kGramSlices - 1) / kGramSlices;
  const int64_t k0 = (int64_t)blockIdx.z * per, k1 = (k0 + per < steps) ? k0 + per : steps;
  v4d acc[2][2] = {{{0, 0, 0, 0}, {0, 0, 0, 0}}, {{0, 0, 0, 0}, {0, 0, 0, 0}}};
  const int i = lane & 15, k = lane >> 4;
  for (int64_t q = k0; q < k1; ++q) {
    const double* __restrict__ row = Z + (q * 4 + k) * Sp;
    const double fa0 = row[a0 + i], fa1 = row[a0 + 16 + i];
    const double fb0 = row[b0 + i], fb1 = row[b0 + 16 + i];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb1, acc[1][1], 0, 0, 0);
  }
  double* __restrict__ out = part + (int64_t)blockIdx.z * Sp * Sp;
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ra = a0 + 16 * ta + (lane >> 4) + 4 * r, cb = b0 + 16 * tb + (lane & 15);
        out[ra * Sp + cb] = acc[ta][tb][r];
      }
}
__global__ void __launch_bounds__(256)
k_rc_gram_sum(const double* __restrict__ part, int64_t Sp, double* __restrict__ G, int64_t row0, double* __restrict__ diag)
{
  // rows row0 .. row0 + gridDim.y - 1 of G (written at G[(a - row0) * Sp + b]); with gridDim.y == 1 and diag != NULL: the diagonal
  if (diag) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= Sp) return;
    double s = 0.0;
    for (int z = 0; z < kGramSlices; ++z) s += part[(int64_t)z * Sp * Sp + b * Sp + b];
    diag[b] = s;
    return;
  }
  const int64_t a = row0 + blockIdx.y, b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= Sp) return;
  const int64_t hi = a > b ? a : b, lo = a > b ? b : a;    // the stored triangle: block row >= block column (diagonal blocks are whole)
  double s = 0.0;
  for (int z = 0; z < kGramSlices; ++z) s += part[(int64_t)z * Sp * Sp + hi * Sp + lo];
  G[(a - row0) * Sp + b] = s;
}

// Per test t (a wave): the K candidates of highest correlation c[r] = G[t][r] / sqrt(G[r][r] G[t][t]), r != t, in R's
// order(decreasing = TRUE) order -- stable (equal values keep the column order), NaN last -- i.e. R/optimize_reference_set.R:101-102 cut
// to the K prefixes that are ever formed.  Round 4 copied the S x S block to the host (8 MB, pageable) and partial-sorted there on 16
// threads: 2.6 ms of the leg.  K rounds of: every lane's best among its untaken columns, a wave reduction under the total order,
// the winner marked.  The correlation is formed as the host formed it (one multiplication, one square root, one division, all
// correctly rounded): the same bits, hence the same order.  c_out (optional): the full rows, for callers that ask for the matrix.
__global__ void __launch_bounds__(64)
k_rc_topk(const double* __restrict__ G, const double* __restrict__ Gd, int64_t S, int64_t Sp, int64_t tb, int K, int32_t* __restrict__ order,
          double* __restrict__ corr_sorted, double* __restrict__ c_out)
{
  extern __shared__ double rc_c[];                  // [S] correlations, then [S] bytes "taken"
  unsigned char* taken = reinterpret_cast<unsigned char*>(rc_c + S);
  const int lane = threadIdx.x;
  const int64_t tl = blockIdx.x, t = tb + tl;
  const double gt = Gd[t];
  for (int64_t r = lane; r < S; r += 64) {
    const double c = G[tl * Sp + r] / __builtin_sqrt(Gd[r] * gt);
    rc_c[r] = c;
    taken[r] = (r == t) ? 1 : 0;
    if (c_out) c_out[tl * S + r] = c;
  }
  __syncthreads();
  auto better = [](double ca, int64_t ia, double cb, int64_t ib) {      // a sorts before b
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    const bool na = ca != ca, nb = cb != cb;
    if (na != nb) return nb;
    if (na) return ia < ib;
    if (ca != cb) return ca > cb;
    return ia < ib;
  };
  for (int k = 0; k < K; ++k) {
    double bc = 0.0;
    int64_t bi = -1;
    for (int64_t r = lane; r < S; r += 64)
      if (!taken[r] && better(rc_c[r], r, bc, bi)) { bc = rc_c[r]; bi = r; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double oc = __shfl_xor(bc, d, 64);
      const int64_t oi = __shfl_xor(bi, d, 64);
      if (better(oc, oi, bc, bi)) { bc = oc; bi = oi; }
    }
    if (lane == 0) { order[tl * K + k] = (int32_t)bi; corr_sorted[tl * K + k] = bc; }
    if (bi >= 0 && lane == (int)(bi & 63)) taken[bi] = 1;
    __syncthreads();
  }
}

// cumulative references of a chunk of tests: cum[e][i * T + j] = sum_{k <= i} X[e][order[(t0 + j) * K + k]], i < K, j < T
__global__ void __launch_bounds__(256)
k_rc_prefix(const int32_t* __restrict__ X, const int32_t* __restrict__ order, int64_t n, int64_t S, int64_t t0, int64_t T, int K,
            int32_t* __restrict__ cum)
{
  extern __shared__ int32_t row[];                       // X[e][0 .. S)
  const int64_t e = blockIdx.x;
  for (int64_t s = threadIdx.x; s < S; s += 256) row[s] = X[e * S + s];
  __syncthreads();
  for (int64_t j = threadIdx.x; j < T; j += 256) {
    const int32_t* __restrict__ o = order + (t0 + j) * K;
    int32_t acc = 0;
    for (int i = 0; i < K; ++i) {
      acc += row[o[i]];
      cum[e * (int64_t)K * T + (int64_t)i * T + j] = acc;
    }
  }
}

// RatioSd numerator with a test column per column: sum_e sqrt(1 + (test + reference_i - 1) phi)  (R/optimize_reference_set.R:128)
__global__ void __launch_bounds__(kWave * kFitSub)
k_rc_ratiosd(const int32_t* __restrict__ cum, const int32_t* __restrict__ X, int64_t S, int64_t t0, int64_t T, int64_t n, int64_t R,
             const double* __restrict__ phi, double* __restrict__ partial, const int* __restrict__ skip_from)
{
  const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int sub = threadIdx.y;
  const int64_t chunk = (int64_t)blockIdx.y * kFitSub + sub;
  if (r >= R) return;
  if (skip_from && (int)(r / T) >= skip_from[r % T]) {      // a prefix the fit skipped: its row of the table is never looked at
    double* o = partial + (chunk * kRsQ) * R + r;
    o[0] = 0; o[R] = 0; o[2 * R] = 0; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
    return;
  }
  const int64_t e0 = (int64_t)blockIdx.y * kFitChunk + sub * (kFitChunk / kFitSub);
  const int64_t e1 = min(e0 + kFitChunk / kFitSub, n);
  const double ph = phi[r];
  const int64_t tc = t0 + r % T;
  double a0 = 0.0;
  int64_t e = e0;
  for (; e + 8 <= e1; e += 8) {       // (eight rows in flight; the sums are added in row order as before)
    int32_t xv[8], cv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { xv[u] = X[(e + u) * S + tc]; cv[u] = cum[(e + u) * R + r]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) a0 += __builtin_sqrt(1.0 + ((double)xv[u] + (double)cv[u] - 1.0) * ph);
  }
  for (; e < e1; ++e)
    a0 += __builtin_sqrt(1.0 + ((double)X[e * S + tc] + (double)cum[e * R + r] - 1.0) * ph);
  double* o = partial + (chunk * kRsQ) * R + r;
  o[0] = a0; o[R] = 0; o[2 * R] = 0; o[3 * R] = 0; o[4 * R] = 0; o[5 * R] = 0;
}

// one sample's column out of the matrix: test[e] = counts[e][t], refs[e][.] = the other S - 1 columns in order
__global__ void __launch_bounds__(256)
k_rc_split_column(const int32_t* __restrict__ counts, int64_t E, int64_t S, int64_t t, int32_t* __restrict__ test, int32_t* __restrict__ refs)
{
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  for (int64_t e = blockIdx.y; e < E; e += gridDim.y) {
    const int32_t v = counts[e * S + s];
    if (s == t) test[e] = v;
    else refs[e * (S - 1) + (s < t ? s : s - 1)] = v;
  }
}

// the test columns of a chunk in the chunk's own order: Xp[e][j] = X[e][tests[j]]
__global__ void __launch_bounds__(256)
k_rc_gather_cols(const int32_t* __restrict__ X, const int32_t* __restrict__ tests, int64_t n, int64_t S, int64_t T, int32_t* __restrict__ Xp)
{
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= T) return;
  const int64_t c = tests[j];
  for (int64_t e = blockIdx.y; e < n; e += gridDim.y) Xp[e * T + j] = X[e * S + c];
}
// ---- the chunk loop in COLUMN-MAJOR form (round 6) ------------------------------------------------------------------------------------------
// Everything select.reference.set needs of a cumulative reference -- the fit (R/optimize_reference_set.R:117-126), the median depth (:127) and RatioSd
// (:128) -- is a function of the column's three count histograms (test y, reference r, total n = y + r).  With the columns laid out one after the other
// (cumT[column][bin], from the transposed counts XT[sample][bin]) ONE workgroup reads its column once, coalesced, and does all of it out of LDS:
//   fit      the gradient and Hessian of the log-likelihood are sums over cells of psi(a + y) - psi(a) = sum_{k < y} 1 / (a + k) (and psi'), i.e. sums over k
//            of T_y(k) / (a + k) with T_y(k) = the number of cells with y > k -- the histograms' TAIL counts, formed once.  A Newton iteration is then one
//            reciprocal and two multiply-adds per occupied bin (~11 000 for a column of 10 000 cells at 100 reads per exon and sample) instead of three
//            digamma / trigamma pairs per cell (~150 instructions), all iterations inside the launch, to a step of 1e-7 (the row-major passes stop at 2e-5).
//            No cancellation between psi values of order log(count): the sums are of positive terms.  Same model, same Newton step (fit_newton_step);
//            the sums are grouped by value instead of by row: the fits agree to rounding (tests/test_gpu_refcohort.py: the single-test entry keeps the
//            row-major passes).
//   median   the two middle order statistics of r from T_r (a binary search)
//   RatioSd  sum_v (#cells with n = v) sqrt(1 + (v - 1) phi), from T_n
// Counts beyond the bins (16 bits wide; two geometries, below) are kept as values (up to 1 024 per coordinate, 16 bits each, sorted, so
// that the order of the sums never depends on timing) and take the bins' whole range plus an asymptotic remainder; a column with more of them, or more than
// 65 535 bins, raises a flag and the chunk is redone by the row-major kernels below (k_rc_prefix ... k_rc_ratiosd), which remain the general path.
// Row-major, these steps were 7.7 of the entry's 11.5 ms at 1 024 samples x 10 000 bins (k_rc_prefix 0.45, the fit 4.2, the medians' bisection 1.5,
// k_rc_ratiosd 0.3, launches and three host round trips between them).
// Two geometries (struct ColGeo): 2 048 / 10 240 / 10 240 bins (y / r / n) for 512 threads, three workgroups per CU -- cohorts of ~100 reads per exon and
// sample, where the deepest cumulative reference a loop reaches holds ~25 samples; and 4 096 / 34 816 / 34 816 bins for 1 024 threads, the CU's whole LDS --
// 3.4 times as deep.  The host picks from the column sums (mean depth of the deepest reachable prefix x 2), a raised flag moves on to the next one.
template <int NT_, int KY_, int KR_, int MINW_> struct ColGeo { static constexpr int NT = NT_, KY = KY_, KR = KR_, KN = KR_, MINW = MINW_; };
using ColSmall = ColGeo<512, 2048, 10240, 6>;
using ColBig = ColGeo<1024, 4096, 34816, 4>;

// XT[s][e] = X[e][s] (pitch np ints per sample)
__global__ void __launch_bounds__(256)
k_rc_transpose(const int32_t* __restrict__ X, int64_t n, int64_t S, int64_t np, int32_t* __restrict__ XT)
{
  __shared__ int32_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t e0 = (int64_t)blockIdx.y * 32, s0 = (int64_t)blockIdx.x * 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t e = e0 + ty + 8 * k, sx = s0 + tx;
    tile[ty + 8 * k][tx] = (e < n && sx < S) ? X[e * S + sx] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t sx = s0 + ty + 8 * k, e = e0 + tx;
    if (sx < S && e < np) XT[sx * np + e] = tile[tx][ty + 8 * k];
  }
}

// cumT[(i * T + j)][e] = sum_{k <= i} XT[order[(t0 + j) * K + k]][e] for the prefixes the loop can reach (i < skip_from[j]), as 16-bit words saturating at 65 535
__global__ void __launch_bounds__(256)
k_rc_prefix_t(const int32_t* __restrict__ XT, const int32_t* __restrict__ order, const int* __restrict__ skip_from, int64_t n, int64_t np, int64_t t0,
              int64_t T, int K, uint16_t* __restrict__ cumT)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (e >= n) return;
  const int kmax = min(K, skip_from[j]);
  const int32_t* __restrict__ ord = order + (t0 + j) * K;
  int32_t acc = 0;
  bool held = true;                                       // (a negative entry is not a count: the column reads "not held" from there on)
  for (int k = 0; k < kmax; ++k) {
    const int32_t x = XT[(int64_t)ord[k] * np + e];
    held = held && x >= 0;
    acc += x;
    cumT[((int64_t)k * T + j) * np + e] = (uint16_t)(held ? min(acc, 65535) : 65535);   // (16 bits: half the bytes; 65 535 = "not held", which k_rc_column's bins and lists refuse)
  }
}

// (col_sum6, col_tails, col_tail_sums, col_sort: csrc/edfit_col.inc -- shared with the samples' own fit, k_fit_col_sm)

// flags: [0] a column the LARGE bins could not hold (the chunk goes to the row-major kernels); [1] fits that ran out of iterations; [2] .. [5] diagnostics;
// [6] the length of the large geometry's list (the host's prediction, plus the columns the small geometry hands on: `redo`)
template <class G>
__device__ __forceinline__ void col_one(const int64_t r, const int32_t* __restrict__ XT, const uint16_t* __restrict__ cumT, const int32_t* __restrict__ perm,
                                        const int* __restrict__ skip_from, int64_t n, int64_t np, int64_t T, int K, double* __restrict__ phi_out,
                                        double* __restrict__ p_out, double* __restrict__ rsd_out, int32_t* __restrict__ med_out, int32_t* __restrict__ redo,
                                        int* __restrict__ flags)
{
  constexpr int kColThreads = G::NT, kColKy = G::KY, kColKr = G::KR, kColKn = G::KN;
  static_assert(kColKy % 4 == 0 && kColKr % 4 == 0 && kColKn % 4 == 0, "four bins per step of the tail sums");
  __shared__ uint32_t s_bins[(kColKy + kColKr + kColKn) / 2];
  __shared__ uint16_t s_ov[3][kColOv];
  __shared__ double s_red[6][kColThreads / 64];
  __shared__ uint32_t s_w[kColThreads / 64];
  __shared__ int s_wm[3][kColThreads / 64];
  __shared__ int s_nov[3];
  __shared__ int s_med[2];
  __shared__ double s_par[4];
  const int tid = threadIdx.x;
  const int64_t R = (int64_t)K * T;
  const int64_t i = r / T, j = r % T;
  if ((int)i >= skip_from[j]) {                          // a prefix the loop never reaches
    if (tid == 0) { phi_out[r] = ed_pm_nan(); p_out[r] = ed_pm_nan(); rsd_out[r] = 0.0; med_out[r] = 0; med_out[R + r] = 0; }
    return;
  }
  uint16_t* const hy = (uint16_t*)s_bins;
  uint16_t* const hr = hy + kColKy;
  uint16_t* const hn = hr + kColKr;
  for (int k = tid; k < (kColKy + kColKr + kColKn) / 2; k += kColThreads) s_bins[k] = 0;
  for (int k = tid; k < 3 * kColOv; k += kColThreads) (&s_ov[0][0])[k] = 0xffff;
  if (tid < 3) s_nov[tid] = 0;
  __syncthreads();
  // ---- one pass over the column: bins, moments ----
  const int32_t* __restrict__ ycol = XT + (int64_t)perm[j] * np;
  const uint16_t* __restrict__ rcol = cumT + r * np;
  double m[6] = {0, 0, 0, 0, 0, 0};                      // sum y, sum n, sum y^2 / n, #cells with n > 0
  int vmax[3] = {0, 0, 0};
  auto put = [&](int c, int v, int base, int Kb) {
    if (v < Kb) atomicAdd(&s_bins[(base + v) >> 1], 1u << (((base + v) & 1) * 16));
    else { const int at = atomicAdd(&s_nov[c], (v < 65535) ? 1 : kColOv + 1); if (at < kColOv) s_ov[c][at] = (uint16_t)v; }
    vmax[c] = max(vmax[c], v);
  };
  for (int64_t e0 = 0; e0 < n; e0 += 4 * kColThreads) {
    int yv[4], rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = e0 + (int64_t)u * kColThreads + tid;
      yv[u] = (e < n) ? ycol[e] : 0x7fffffff;
      rv[u] = (e < n) ? rcol[e] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (yv[u] == 0x7fffffff) continue;                    // (beyond the last bin)
      const int y = yv[u], rr = rv[u], nn = y + rr;
      if ((y | rr) < 0) { atomicAdd(&s_nov[0], kColOv + 1); continue; }      // a negative count (not a count): the row-major kernels' per-cell arithmetic decides what it means
      put(0, y, 0, kColKy); put(1, rr, kColKy, kColKr); put(2, nn, kColKy + kColKr, kColKn);
      if (nn > 0) { m[0] += (double)y; m[1] += (double)nn; m[2] += ((double)y * (double)y) / (double)nn; m[3] += 1.0; }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) vmax[c] = max(vmax[c], __shfl_xor(vmax[c], d, 64));
    if ((tid & 63) == 0) s_wm[c][tid >> 6] = vmax[c];
  }
  col_sum6<kColThreads>(m, s_red, tid);                               // (its barriers publish s_wm too)
  int ylim = 0, rlim = 0, nlim = 0;
  for (int w = 0; w < kColThreads / 64; ++w) { ylim = max(ylim, s_wm[0][w]); rlim = max(rlim, s_wm[1][w]); nlim = max(nlim, s_wm[2][w]); }
  // the bins that can hold a count: [0, largest value] -- T(k) = 0 from the largest value on
  ylim = min(ylim + 1, kColKy); rlim = min(rlim + 1, kColKr); nlim = min(nlim + 1, kColKn);
  const int novy = s_nov[0], novr = s_nov[1], novn = s_nov[2];
  if (tid == 0 && (novy | novr | novn)) { atomicMax(&flags[2], max(novy, max(novr, novn))); atomicAdd(&flags[3], 1); }    // (diagnostics: ED_REFCOHORT_TIMING)
  if (novy > kColOv || novr > kColOv || novn > kColOv) {            // (uniform) more than the lists keep: the next form's
    if (tid == 0) {
      if (redo) redo[atomicAdd(&flags[6], 1)] = (int32_t)r;           // (the order of the list decides nothing: a column is a workgroup's own)
      else atomicOr(&flags[0], 1);
    }
    return;
  }
  if (novy) col_sort<kColThreads>(s_ov[0], tid);
  if (novr) col_sort<kColThreads>(s_ov[1], tid);
  if (novn) col_sort<kColThreads>(s_ov[2], tid);
  col_tails<kColThreads>(hy, ylim, (uint32_t)novy, s_w, tid);
  col_tails<kColThreads>(hr, rlim, (uint32_t)novr, s_w, tid);
  col_tails<kColThreads>(hn, nlim, (uint32_t)novn, s_w, tid);
  // ---- the fit: method-of-moments start (k_fit_start's), Newton on the tail sums ----
  double eta_v, lam_v;
  int done_v;
  {
    const double sy = m[0], sn = m[1], syy = m[2], cnt = m[3];
    double p = (sn > 0) ? sy / sn : 0.5;
    p = fmin(fmax(p, 1e-6), 1.0 - 1e-6);
    const double q = 1.0 - p;
    const double pearson = (syy - 2.0 * p * sy + p * p * sn) / (p * q);
    double ph = (sn - cnt > 0) ? (pearson - cnt) / (sn - cnt) : 0.01;
    ph = fmin(fmax(ph, 1e-4), 0.3);
    eta_v = ed_plog(p / q);
    lam_v = ed_plog((1.0 - ph) / ph);
    done_v = (cnt < 2.0) ? 1 : 0;
  }
  int it = 0;
  for (; it < 100 && !done_v; ++it) {
    const double th = ed_pexp(lam_v);
    const double p = 1.0 / (1.0 + ed_pexp(-eta_v));
    const double a = th * p, b = th * (1.0 - p);
    double t[6] = {0, 0, 0, 0, 0, 0};                    // A1, A2 (y, a), B1, B2 (r, b), C1, C2 (n, th)
    col_tail_sums<kColThreads>(hy, ylim, a, t[0], t[1], tid);
    col_tail_sums<kColThreads>(hr, rlim, b, t[2], t[3], tid);
    col_tail_sums<kColThreads>(hn, nlim, th, t[4], t[5], tid);
    // values beyond the bins: the bins took k < K; psi(x + v) - psi(x + K) and psi' remain
    auto beyond = [&](int c, int nov, double x, int Kb, double& s1, double& s2) {
      for (int u = tid; u < nov; u += kColThreads) {
        double p0, q0, p1, q1;
        edfit::digamma_trigamma(x + (double)Kb, p0, q0);
        edfit::digamma_trigamma(x + (double)s_ov[c][u], p1, q1);
        s1 += p1 - p0; s2 += q0 - q1;
      }
    };
    beyond(0, novy, a, kColKy, t[0], t[1]); beyond(1, novr, b, kColKr, t[2], t[3]); beyond(2, novn, th, kColKn, t[4], t[5]);
    col_sum6<kColThreads>(t, s_red, tid);
    if (tid == 0) {
      const double tot[kFitQ] = {t[0] - t[4], t[2] - t[4], t[5] - t[1], t[5], t[5] - t[3], 0.0};
      double e2 = eta_v, l2 = lam_v;
      int d2 = 0;
      fit_newton_step(tot, e2, l2, d2, 1e-7, 1);
      s_par[0] = e2; s_par[1] = l2; s_par[2] = (double)d2;
    }
    __syncthreads();
    eta_v = s_par[0]; lam_v = s_par[1]; done_v = s_par[2] != 0.0;
  }
  const double th = ed_pexp(lam_v);
  const double phi = 1.0 / (th + 1.0);                   // (k_fit_finish)
  // ---- RatioSd's sum over the values of n (R/optimize_reference_set.R:128), all n bins of the column ----
  double sd[6] = {0, 0, 0, 0, 0, 0};
  for (int v = tid; v < nlim; v += kColThreads) {
    const double c = (v == 0) ? (double)n - (double)hn[0] : (double)hn[v - 1] - (double)hn[v];
    if (c != 0.0) sd[0] = __builtin_fma(c, __builtin_sqrt(1.0 + ((double)v - 1.0) * phi), sd[0]);
  }
  for (int u = tid; u < novn; u += kColThreads) sd[0] += __builtin_sqrt(1.0 + ((double)s_ov[2][u] - 1.0) * phi);
  // ---- the order statistics (n - 1) / 2 and n / 2 of r: the smallest v with #(r <= v) = n - T_r(v) >= k + 1, i.e. T_r(v) <= n - k - 1 < T_r(v - 1) ----
  const int64_t need0 = n - (n - 1) / 2 - 1, need1 = n - n / 2 - 1;
  for (int v = tid; v < rlim; v += kColThreads) {
    const int64_t tv = hr[v], tp = v ? (int64_t)hr[v - 1] : n + 1;
    if (tv <= need0 && tp > need0) s_med[0] = v;
    if (tv <= need1 && tp > need1) s_med[1] = v;
  }
  col_sum6<kColThreads>(sd, s_red, tid);
  if (tid == 0) {
    phi_out[r] = phi;
    p_out[r] = 1.0 / (1.0 + ed_pexp(-eta_v));
    rsd_out[r] = sd[0];
    if (it >= 100 && !done_v) atomicAdd(&flags[1], 1);
    atomicAdd(&flags[4], it);
    atomicMax(&flags[5], it);
    // (a statistic among the values beyond the bins: they are sorted)
    med_out[r] = ((int64_t)novr > need0) ? (int32_t)s_ov[1][(n - 1) / 2 - (n - (int64_t)novr)] : s_med[0];
    med_out[R + r] = ((int64_t)novr > need1) ? (int32_t)s_ov[1][n / 2 - (n - (int64_t)novr)] : s_med[1];
  }
}

// The small geometry: workgroup b takes column list[b], b < n_list (the host's list).  The large geometry: a persistent grid walks list[0 .. flags[6]) --
// the host's prediction followed by what the small geometry's launch, earlier on the same stream, handed on.
template <class G>
__global__ void __launch_bounds__(G::NT, G::MINW)       // (small geometry: 6 waves per SIMD = three workgroups per CU, what the LDS allows -- 85 registers)
k_rc_column(const int32_t* __restrict__ XT, const uint16_t* __restrict__ cumT, const int32_t* __restrict__ perm /* + t0 */, const int* __restrict__ skip_from,
            int64_t n, int64_t np, int64_t T, int K, double* __restrict__ phi_out, double* __restrict__ p_out, double* __restrict__ rsd_out,
            int32_t* __restrict__ med_out /* [2][R] */, const int32_t* __restrict__ list, int n_list /* < 0: flags[6] */, int32_t* __restrict__ redo,
            int* __restrict__ flags)
{
  if (n_list >= 0) {
    if ((int)blockIdx.x < n_list) col_one<G>(list[blockIdx.x], XT, cumT, perm, skip_from, n, np, T, K, phi_out, p_out, rsd_out, med_out, redo, flags);
    return;
  }
  const int nl = *(volatile int*)&flags[6];
  for (int c = blockIdx.x; c < nl; c += gridDim.x) {
    col_one<G>(list[c], XT, cumT, perm, skip_from, n, np, T, K, phi_out, p_out, rsd_out, med_out, redo, flags);
    __syncthreads();                                    // (the LDS is the next column's)
  }
}

// brackets of the prefixes the fit skipped (k_fit_skip_prefixes) closed before the search starts: their columns cost nothing
__global__ void k_rc_close_skipped(const int* __restrict__ skip_from, int K, int64_t T, int32_t* __restrict__ lo, int32_t* __restrict__ hi)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (int64_t)K * T) return;
  if ((int)(r / T) >= skip_from[r % T]) { lo[r] = 0; hi[r] = 0; }
}

// the aggregate reference of every sample, all exons: ref[e][t] = sum_{k < n_chosen[t]} counts[e][choice[t * K + k]].
// A thread owns one sample and keeps its list of chosen columns in registers (32 at a time) while the workgroup walks its share of
// the rows in tiles staged in LDS (all S candidate columns of `rows` rows): the gathers are LDS reads only.  (One row per
// workgroup with the lists re-read from memory for every row was 4.2 ms at 200 000 x 1024.)
constexpr int kAggList = 32;
constexpr int kAggRowsMax = 16;
__global__ void __launch_bounds__(256)
k_rc_aggregate(const int32_t* __restrict__ counts, const int32_t* __restrict__ choice, const int32_t* __restrict__ n_chosen, int64_t E,
               int64_t S, int K, int rows, int64_t rows_per_wg, int32_t* __restrict__ ref, int64_t Sr /* tests = columns of ref (<= S) */)
{
  extern __shared__ int32_t tile[];   // [rows][S]
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < Sr;
  const int nc = live ? min(n_chosen[t], K) : 0;
  const int64_t e_begin = (int64_t)blockIdx.y * rows_per_wg, e_end = min(e_begin + rows_per_wg, E);
  for (int64_t e0 = e_begin; e0 < e_end; e0 += rows) {
    const int nr = (int)min((int64_t)rows, e_end - e0);
    __syncthreads();   // the previous tile's readers are done
    for (int64_t i = threadIdx.x; i < (int64_t)nr * S; i += 256) tile[i] = counts[e0 * S + i];
    __syncthreads();
    int32_t acc[kAggRowsMax];
#pragma unroll
    for (int r = 0; r < kAggRowsMax; ++r) acc[r] = 0;
    for (int k0 = 0; k0 < nc; k0 += kAggList) {
      int idx[kAggList];
#pragma unroll
      for (int k = 0; k < kAggList; ++k) idx[k] = (k0 + k < nc) ? choice[t * K + k0 + k] : -1;
#pragma unroll
      for (int r = 0; r < kAggRowsMax; ++r) {
        if (r < nr) {
          const int32_t* __restrict__ row = tile + (int64_t)r * S;
          int32_t a = 0;
#pragma unroll
          for (int k = 0; k < kAggList; ++k) a += (idx[k] >= 0) ? row[idx[k]] : 0;
          acc[r] += a;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < kAggRowsMax; ++r)
        if (r < nr) ref[(e0 + r) * Sr + t] = acc[r];
    }
  }
}

// The same sums written SAMPLE-MAJOR, ref_sm[t][e] -- the layout the table-driven emission mode works in (R's column-major matrix) -- and,
// on request, the count matrix itself transposed alongside (counts_sm[s][e]): the tile is in LDS anyway.  Lanes run over ROWS here: a
// group of R lanes owns one test, its lanes the tile's R rows; the chosen column is uniform over the group, so an LDS read is R
// consecutive words (tile[column][row], column stride R + 1 words: no bank conflicts, where k_rc_aggregate's 64 lanes gather 64 random
// columns of a row) and only the test's own n_chosen columns are read (not a fixed 32); a store is R x 4 contiguous bytes of a row of
// ref_sm.  A PERSISTENT grid (one workgroup per CU) walks the tiles, with every test's list in LDS as 16-bit words, loaded once: a
// first form that fetched a test's list from memory inside the tile loop spent its time waiting for those loads (5.8 ms; this: DESIGN 4.6).
constexpr int kAggSmThreads = 1024;
__global__ void __launch_bounds__(kAggSmThreads)
k_rc_aggregate_sm(const int32_t* __restrict__ counts, const int32_t* __restrict__ choice, int64_t E, int64_t S, int K, int R /* rows per tile: 32, 16 or 8 */,
                  int32_t* __restrict__ ref_sm, int64_t Sr, int32_t* __restrict__ counts_sm)
{
  extern __shared__ int32_t agg_lds[];   // tile [S][R + 1] int32, then lists [Sr][K] uint16 (0xffff = none)
  const int Rp = R + 1;
  int32_t* tile = agg_lds;
  unsigned short* lists = reinterpret_cast<unsigned short*>(agg_lds + ((S * Rp + 3) & ~(int64_t)3));     // (16-byte aligned: read as uint4)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K8 = (K + 7) & ~7;               // a test's list padded to whole groups of eight 16-bit words (one 16-byte LDS read)
  for (int64_t i = tid; i < Sr * K8; i += kAggSmThreads) {
    const int64_t t = i / K8;
    const int k = (int)(i - t * K8);
    const int32_t c = (k < K) ? choice[t * K + k] : -1;
    lists[i] = (c >= 0) ? (unsigned short)c : (unsigned short)0xffffu;
  }
  const int per = 64 / R;                    // tests per wave and turn (2, 4 or 8)
  const int row = lane % R, sub = lane / R;
  const int64_t ntile = (E + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
    const int64_t e0 = tl * R;
    const int nr = (int)min((int64_t)R, E - e0);
    __syncthreads();          // the previous tile's readers are done (first turn: the lists are complete)
    if ((S & 3) == 0) {       // staging: the tile is nr x S consecutive words of counts; 16-byte loads, eight in flight per thread before any is parked
      const int64_t S4 = S >> 2, n4 = (int64_t)nr * S4;
      const int4* __restrict__ src = reinterpret_cast<const int4*>(counts + e0 * S);
      for (int64_t base = 0; base < n4; base += (int64_t)8 * kAggSmThreads) {
        int4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int64_t i = base + (int64_t)j * kAggSmThreads + tid;
          v[j] = (i < n4) ? src[i] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int64_t i = base + (int64_t)j * kAggSmThreads + tid;
          if (i < n4) {
            const int64_t r = i / S4, q = i - r * S4;
            int32_t* o = tile + (q * 4) * Rp + r;
            o[0] = v[j].x; o[Rp] = v[j].y; o[2 * Rp] = v[j].z; o[3 * Rp] = v[j].w;
          }
        }
      }
    } else {
      for (int r = 0; r < nr; ++r)
        for (int64_t sidx = tid; sidx < S; sidx += kAggSmThreads) tile[sidx * Rp + r] = counts[(e0 + r) * S + sidx];
    }
    __syncthreads();
    const bool rlive = row < nr;
    for (int64_t t0 = (int64_t)wave * per; t0 < Sr; t0 += (int64_t)(kAggSmThreads / 64) * per) {
      const int64_t t = t0 + sub;
      const bool live = t < Sr;
      // eight columns per step: one 16-byte read of the list, then eight independent reads of the tile (a column at a time was a chain of
      // two dependent LDS round trips per column with two waves per SIMD to hide them)
      const uint4* __restrict__ lst = reinterpret_cast<const uint4*>(lists + (live ? t : 0) * K8);
      int32_t acc = 0;
      for (int g = 0; g < K8 / 8; ++g) {
        uint4 w = lst[g];
        if (!live) w = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        if (__builtin_amdgcn_ballot_w64((w.x & 0xffffu) != 0xffffu) == 0ull) break;      // every test of the wave has run out of columns (-1 padded lists)
        const unsigned c[8] = {w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16, w.z & 0xffffu, w.z >> 16, w.w & 0xffffu, w.w >> 16};
        int32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = tile[(int64_t)(c[q] != 0xffffu ? c[q] : 0u) * Rp + row];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += (c[q] != 0xffffu) ? v[q] : 0;
      }
      if (live && rlive) ref_sm[t * E + e0 + row] = acc;
    }
    if (counts_sm) {
      for (int64_t s0 = (int64_t)wave * per; s0 < S; s0 += (int64_t)(kAggSmThreads / 64) * per) {
        const int64_t sidx = s0 + sub;
        if (sidx < S && rlive) counts_sm[sidx * E + e0 + row] = tile[sidx * Rp + row];
      }
    }
  }
}

// coverage guard of select.reference.set (R/optimize_reference_set.R:57-61) for every column at once: bins with more than 2 reads
__global__ void __launch_bounds__(256)
k_rc_count_gt2(const int32_t* __restrict__ counts, int64_t E, int64_t S, int64_t rows_per, int* __restrict__ out)
{
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const int64_t e0 = (int64_t)blockIdx.y * rows_per, e1 = min(e0 + rows_per, E);
  int c = 0;
  for (int64_t e = e0; e < e1; ++e) c += counts[e * S + s] > 2 ? 1 : 0;
  if (c) atomicAdd(&out[s], c);
}

// Small transfers that do not go through the DMA engines.  The entry makes ~25 host <-> device copies of a few KB to 1.6 MB each; as
// hipMemcpyAsync they queue on the copy engines, in order, behind whatever the process has there -- with the NEXT cohort's counts (410 MB)
// crossing the link on another stream, the first of them waited for all of it (bench.py's back-to-back cohorts: the reference-set stage
// 26.5 ms instead of 16.7, exactly the upload).  Here a kernel moves the words between device memory and a pinned, device-visible host
// block (grow-only, kept with the scratch): host -> device = memcpy into the block + a kernel that reads it over the link; device -> host
// = a kernel that writes the block + a memcpy out of it after the next synchronisation (RcLink::sync replaces hipStreamSynchronize
// wherever results are awaited).  Transfers that do not fit the block fall back to hipMemcpyAsync.
__global__ void __launch_bounds__(256)
k_link_copy(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n_words)
{
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
struct RcLink {
  PinBuf<char> up;   size_t up_used = 0;       // host -> device staging (pinned)
  PinBuf<char> down; size_t down_used = 0;     // device -> host staging (pinned)
  struct Pending { void* dst; const char* src; size_t bytes; };
  std::vector<Pending> pending;
  void release() { up.reset(); down.reset(); up_used = down_used = 0; pending.clear(); }
  int begin(size_t cap)       // start of a call: both blocks there (or not: everything then goes through hipMemcpyAsync), nothing pending
  {
    up_used = down_used = 0; pending.clear();
    if (!up && up.alloc(cap) != hipSuccess) (void)hipGetLastError();
    if (!down && down.alloc(cap) != hipSuccess) (void)hipGetLastError();
    return ED_OK;
  }
  static unsigned blocks_for(size_t words) { return (unsigned)std::max<size_t>(1, std::min<size_t>(256, (words + 1023) / 1024)); }
  int put(void* d_dst, const void* h_src, size_t bytes, hipStream_t st)
  {
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (bytes == 0) return ED_OK;
    if ((bytes & 3) || !up || up_used + need > up.bytes()) { HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, st)); return ED_OK; }
    char* q = up + up_used; up_used += need;         // (a region is written once per call: the kernel that reads it may still be queued)
    std::memcpy(q, h_src, bytes);
    hipLaunchKernelGGL(k_link_copy, dim3(blocks_for(bytes / 4)), dim3(256), 0, st, (const uint32_t*)q, (uint32_t*)d_dst, bytes / 4);
    return ED_OK;
  }
  int get(void* h_dst, const void* d_src, size_t bytes, hipStream_t st)     // h_dst is complete after the next sync()
  {
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (bytes == 0) return ED_OK;
    if ((bytes & 3) || !down || down_used + need > down.bytes()) { HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st)); return ED_OK; }
    char* q = down + down_used; down_used += need;
    hipLaunchKernelGGL(k_link_copy, dim3(blocks_for(bytes / 4)), dim3(256), 0, st, (const uint32_t*)d_src, (uint32_t*)q, bytes / 4);
    pending.push_back({h_dst, q, bytes});
    return ED_OK;
  }
  int sync(hipStream_t st)
  {
    HIP_TRY(hipStreamSynchronize(st));
    for (const Pending& x : pending) std::memcpy(x.dst, x.src, x.bytes);
    pending.clear(); down_used = 0;
    return ED_OK;
  }
};

// Device scratch of ed_cohort_select_reference_sets, kept between calls (grow-only, handed out in call order): the entry makes ~35
// allocations, 1.3 GB the largest, and freeing them synchronises the device -- 2-4 ms per call as a rule and 10 ms when the driver
// unmaps (seen as an outlier of the phase timer).  One call at a time uses it (a mutex); ed_release_scratch() gives it back.
struct RcScratch {
  std::mutex mu;
  std::vector<DevBuf<void>> bufs;     // grow-only, handed out in call order
  size_t next = 0;
  int device = -1;
  FitWork fw;
  int64_t fw_E = 0, fw_S = 0;
  RcLink link;
  void release_all()
  {
    bufs.clear(); next = 0;
    fw = FitWork(); fw_E = fw_S = 0;
    link.release();
  }
  hipError_t get(void** p, size_t bytes)
  {
    if (next == bufs.size()) bufs.emplace_back();
    DevBuf<void>& b = bufs[next++];
    const hipError_t e = b.reserve(bytes);
    *p = b.get();
    return e;
  }
  int fit_work(int64_t E, int64_t S, FitWork** out)
  {
    if (fw_E < E || fw_S < S || !fw.partial) {
      if (int rc = fw.alloc(std::max(E, fw_E), std::max(S, fw_S))) { fw_E = fw_S = 0; return rc; }
      fw_E = std::max(E, fw_E); fw_S = std::max(S, fw_S);
    }
    *out = &fw;
    return ED_OK;
  }
};
RcScratch& g_rc_scratch = *new RcScratch;     // (never destroyed at exit: the HIP runtime may be gone by then; ed_release_scratch() gives the memory back)
// how the last call's chunks were served (under the scratch mutex): chunks by k_rc_column, chunks left to the row-major kernels, columns with counts
// beyond the bins, the largest number of Newton iterations of a column, columns served by the large geometry -- ed_refcohort_last_path
int64_t g_rc_last_path[5] = {0, 0, 0, 0, 0};
struct PoolBuf {
  void* p = nullptr;
  hipError_t alloc(size_t bytes) { return g_rc_scratch.get(&p, bytes); }
  template <class T> T* as() { return (T*)p; }
};

}  // namespace

static int refcohort_impl(const int32_t* d_counts, int64_t n_bins, int64_t n_samples, const double* bin_length,
                          int64_t n_bins_reduced, int32_t max_refs, int64_t test_begin, int64_t test_end,
                          int32_t* n_chosen, int32_t* choice, ed_refset_row* rows, double* correlations,
                          int32_t* d_ref_out, int64_t* n_selected_bins, void* stream_, int32_t* d_ref_sm_out, int32_t* d_counts_sm_out)
{
  if (!d_counts || !n_chosen || !choice || n_bins <= 0 || n_samples < 2)
    return ed_fail(ED_ERR_INVALID, "ed_cohort_select_reference_sets: bad arguments (at least 2 samples)");
  if (test_begin < 0 || test_end > n_samples || test_begin >= test_end)
    return ed_fail(ED_ERR_INVALID, "ed_cohort_select_reference_sets_range: tests [%lld, %lld) of %lld samples", (long long)test_begin, (long long)test_end,
                   (long long)n_samples);
  const int64_t tb = test_begin, te = test_end, Sr = te - tb;     // the tests of this call; every sample is a candidate
  if (n_samples > 16384) return ed_fail(ED_ERR_INVALID, "ed_cohort_select_reference_sets: at most 16384 samples per call");
  if (int rc = require_device()) return rc;
  std::lock_guard<std::mutex> scratch_lock(g_rc_scratch.mu);
  {
    int dev_now = 0;
    (void)hipGetDevice(&dev_now);
    if (g_rc_scratch.device != dev_now) { g_rc_scratch.release_all(); g_rc_scratch.device = dev_now; }
    g_rc_scratch.next = 0;
  }
  for (int q = 0; q < 5; ++q) g_rc_last_path[q] = 0;
  hipStream_t st = (hipStream_t)stream_;
  RcLink& link = g_rc_scratch.link;
  link.begin((size_t)16 << 20);
  const int64_t E = n_bins, S = n_samples;
  const int K = (int)std::min<int64_t>(max_refs > 0 ? max_refs : 32, S - 1);
  const bool tick_on = getenv("ED_REFCOHORT_TIMING") != nullptr;   // (diagnostic) wall time of the phases, to stderr
  auto tick_t0 = std::chrono::steady_clock::now();
  auto tick = [&](const char* what) {
    if (!tick_on) return;
    (void)hipStreamSynchronize(st);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[refcohort] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tick_t0).count());
    tick_t0 = now;
  };
  if (bin_length)
    for (int64_t e = 0; e < E; ++e)
      if (bin_length[e] == 0) return ed_fail(ED_ERR_INVALID, "bin.length contains zeros. All bin lengths must be positive");
  for (int64_t t = 0; t < Sr; ++t) n_chosen[t] = 0;
  for (int64_t i = 0; i < Sr * K; ++i) choice[i] = -1;
  // ---- bin selection, shared by every test (R/optimize_reference_set.R:79-97): total = row sums over ALL samples ----
  LengthQuantiles lq;
  lq.start(bin_length, E);       // (host threads, underneath the row totals and their copy)
  PoolBuf dtotal, dzero;
  HIP_TRY(dtotal.alloc((size_t)E * 8));
  HIP_TRY(dzero.alloc((size_t)E * 4));
  HIP_TRY(hipMemsetAsync(dzero.p, 0, (size_t)E * 4, st));
  hipLaunchKernelGGL(k_rs_rowtotal, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, st, dzero.as<int32_t>(), d_counts, E, S, dtotal.as<double>());
  std::vector<double> total((size_t)E);
  if (int rc = link.get(total.data(), dtotal.p, (size_t)E * 8, st)) return rc;
  if (int rc = link.sync(st)) return rc;
  tick("  row totals + copy");
  // coverage guard per test (:57-61): fewer than 5 bins with more than 2 reads -> the first candidate.  It needs nothing but the
  // counts: issued here, it runs while the host selects the bins (the device would sit idle for that long), and is read further down.
  PoolBuf dcnt_gt2;
  std::vector<int> h_gt2((size_t)S);
  {
    HIP_TRY(dcnt_gt2.alloc((size_t)S * 4));
    HIP_TRY(hipMemsetAsync(dcnt_gt2.p, 0, (size_t)S * 4, st));
    const int64_t rows_per = std::max<int64_t>(512, (E + 59999) / 60000);
    hipLaunchKernelGGL(k_rc_count_gt2, dim3((unsigned)((S + 255) / 256), (unsigned)((E + rows_per - 1) / rows_per)), dim3(256), 0, st, d_counts, E, S,
                       rows_per, dcnt_gt2.as<int>());
    if (int rc = link.get(h_gt2.data(), dcnt_gt2.p, (size_t)S * 4, st)) return rc;
  }
  std::vector<int32_t> sel;
  if (int rc = refset_select_bins(total, bin_length, E, n_bins_reduced, sel, &lq)) return rc;
  const int64_t n = (int64_t)sel.size();
  tick("bin selection");
  if (n_selected_bins) *n_selected_bins = n;
  if (n < 2) return ed_fail(ED_ERR_STATE, "ed_cohort_select_reference_sets: fewer than 2 bins selected");
  const int64_t nblk = (n + kFitChunk - 1) / kFitChunk, nchunk = nblk * kFitSub;
  // ---- the selected bins, compacted; column sums; normalised, centred Z; Gram matrix; correlations ----
  const int64_t Sp = (S + 31) / 32 * 32, n4 = (n + 3) / 4 * 4;
  PoolBuf dsel, dlen, dX, dpart, dred, dcolsum, dcolmean, dZ, dGp, dG;
  HIP_TRY(dsel.alloc((size_t)n * 4));
  if (int rc = link.put(dsel.p, sel.data(), (size_t)n * 4, st)) return rc;
  if (bin_length) {
    HIP_TRY(dlen.alloc((size_t)E * 8));
    if (int rc = link.put(dlen.p, bin_length, (size_t)E * 8, st)) return rc;
  }
  HIP_TRY(dX.alloc((size_t)n * S * 4));
  hipLaunchKernelGGL(k_rc_compact, dim3((unsigned)((S + 255) / 256), (unsigned)n), dim3(256), 0, st, d_counts, dsel.as<int32_t>(), n, S, dX.as<int32_t>());
  std::vector<int32_t> ident((size_t)n);
  for (int64_t e = 0; e < n; ++e) ident[(size_t)e] = (int32_t)e;
  PoolBuf dident;
  HIP_TRY(dident.alloc((size_t)n * 4));
  if (int rc = link.put(dident.p, ident.data(), (size_t)n * 4, st)) return rc;
  const int64_t Rmax_cols = std::max<int64_t>(S, 1);
  HIP_TRY(dpart.alloc((size_t)nchunk * kRsQ * Rmax_cols * 8));
  HIP_TRY(dred.alloc((size_t)kRsQ * Rmax_cols * 8));
  HIP_TRY(dcolsum.alloc((size_t)S * 8));
  HIP_TRY(dcolmean.alloc((size_t)S * 8));
  const dim3 gcol((unsigned)((S + kWave - 1) / kWave), (unsigned)nblk), bcol(kWave, kFitSub), bred(kWave, kRedY);
  std::vector<double> red((size_t)kRsQ * S);
  auto reduce_to_host = [&](PoolBuf& part, PoolBuf& redbuf, std::vector<double>& out, int64_t cols) -> int {
    hipLaunchKernelGGL(k_rs_reduce, dim3((unsigned)((cols + kWave - 1) / kWave)), bred, 0, st, part.as<double>(), nchunk, cols, redbuf.as<double>());
    out.resize((size_t)kRsQ * cols);
    if (int rc = link.get(out.data(), redbuf.p, (size_t)kRsQ * cols * 8, st)) return rc;
    if (int rc = link.sync(st)) return rc;
    return ED_OK;
  };
  hipLaunchKernelGGL(k_rs_colsum, gcol, bcol, 0, st, dX.as<int32_t>(), dident.as<int32_t>(), n, S, dpart.as<double>());
  if (int rc = reduce_to_host(dpart, dred, red, S)) return rc;
  std::vector<double> colsum(red.begin(), red.begin() + S), colmean((size_t)S);
  if (int rc = link.put(dcolsum.p, colsum.data(), (size_t)S * 8, st)) return rc;
  // sums of the normalised counts (mode 0 of k_rs_colmoments: `test` is not read), on the ORIGINAL rows for the bin lengths
  hipLaunchKernelGGL(k_rs_colmoments, gcol, bcol, 0, st, d_counts, (const int32_t*)nullptr, bin_length ? dlen.as<double>() : nullptr,
                     dsel.as<int32_t>(), n, S, dcolsum.as<double>(), 1.0, 0, (const double*)nullptr, 0.0, dpart.as<double>());
  if (int rc = reduce_to_host(dpart, dred, red, S)) return rc;
  for (int64_t s = 0; s < S; ++s) colmean[(size_t)s] = red[(size_t)s] / (double)n;
  if (int rc = link.put(dcolmean.p, colmean.data(), (size_t)S * 8, st)) return rc;
  HIP_TRY(dZ.alloc((size_t)n4 * Sp * 8));
  hipLaunchKernelGGL(k_rc_centre, dim3((unsigned)((Sp + 255) / 256), (unsigned)n4), dim3(256), 0, st, dX.as<int32_t>(), dsel.as<int32_t>(),
                     bin_length ? dlen.as<double>() : nullptr, n, S, dcolsum.as<double>(), dcolmean.as<double>(), Sp, dZ.as<double>());
  PoolBuf dGd;
  HIP_TRY(dGp.alloc((size_t)kGramSlices * Sp * Sp * 8));
  HIP_TRY(dG.alloc((size_t)Sr * Sp * 8));
  HIP_TRY(dGd.alloc((size_t)Sp * 8));
  HIP_TRY(hipMemsetAsync(dGp.p, 0, (size_t)kGramSlices * Sp * Sp * 8, st));
  // rows [tb, te) of the Gram matrix (a (te - tb) x S block when the call covers a share of the tests) and its diagonal
  hipLaunchKernelGGL(k_rc_gram, dim3((unsigned)(Sp / 32), (unsigned)(Sp / 32), (unsigned)kGramSlices), dim3(64), 0, st, dZ.as<double>(), n4, Sp,
                     dGp.as<double>(), tb / 32, (te + 31) / 32);
  hipLaunchKernelGGL(k_rc_gram_sum, dim3((unsigned)((Sp + 255) / 256), (unsigned)Sr), dim3(256), 0, st, dGp.as<double>(), Sp, dG.as<double>(), tb,
                     (double*)nullptr);
  hipLaunchKernelGGL(k_rc_gram_sum, dim3((unsigned)((Sp + 255) / 256), 1), dim3(256), 0, st, dGp.as<double>(), Sp, (double*)nullptr, (int64_t)0,
                     dGd.as<double>());
  // ---- per test: the other samples by decreasing correlation (stable, NaN last: R's order(decreasing = TRUE)), on the device ----
  std::vector<int32_t> order((size_t)Sr * K);          // (per-test arrays are indexed by t - tb from here on)
  std::vector<double> corr_sorted((size_t)Sr * K);
  {
    PoolBuf dord, dcs, dcfull;
    HIP_TRY(dord.alloc((size_t)Sr * K * 4));
    HIP_TRY(dcs.alloc((size_t)Sr * K * 8));
    if (correlations) HIP_TRY(dcfull.alloc((size_t)Sr * S * 8));
    const size_t lds = (size_t)S * 9 + 16;
    if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)k_rc_topk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_rc_topk, dim3((unsigned)Sr), dim3(64), lds, st, dG.as<double>(), dGd.as<double>(), S, Sp, tb, K, dord.as<int32_t>(),
                       dcs.as<double>(), correlations ? dcfull.as<double>() : (double*)nullptr);
    if (int rc = link.get(order.data(), dord.p, order.size() * 4, st)) return rc;
    if (int rc = link.get(corr_sorted.data(), dcs.p, corr_sorted.size() * 8, st)) return rc;
    if (correlations) if (int rc = link.get(correlations, dcfull.p, (size_t)Sr * S * 8, st)) return rc;
    if (int rc = link.sync(st)) return rc;
    HIP_TRY(hipGetLastError());
  }
  tick("correlations + ordering (device)");
  // The tests in the order of where the reference's loop is expected to stop for them (its proportion test on the column sums): the
  // prefixes the fit then skips (k_fit_skip_prefixes) fill whole wavefronts of columns instead of being scattered over all of them --
  // 46 % of the columns were skipped and 8 % of the wavefronts.  The order decides nothing but the layout.
  std::vector<int32_t> perm((size_t)Sr);               // perm[j]: the test (column of the cohort) at position j of this call's layout
  std::vector<int> stop((size_t)Sr, K);                // ... and where its loop is expected to stop: the prefixes from there on are not formed
  {
    for (int64_t t = tb; t < te; ++t) {
      double run = 0.0;
      for (int i = 0; i < K; ++i) {
        run += colsum[(size_t)order[(size_t)((t - tb) * K + i)]];
        const double ph = colsum[(size_t)t] / (colsum[(size_t)t] + run);
        if (i + 1 > 2 && ph < 0.04) { stop[(size_t)(t - tb)] = i + 1; break; }
      }
    }
    for (int64_t t = tb; t < te; ++t) perm[(size_t)(t - tb)] = (int32_t)t;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return stop[(size_t)(a - tb)] > stop[(size_t)(b - tb)]; });
  }
  std::vector<int32_t> order_p((size_t)Sr * K);
  for (int64_t j = 0; j < Sr; ++j) std::memcpy(&order_p[(size_t)(j * K)], &order[(size_t)(((int64_t)perm[(size_t)j] - tb) * K)], (size_t)K * 4);
  tick("layout of the tests (host)");
  std::vector<int64_t> n_gt2((size_t)S, 0);        // (the coverage guard's kernel and copy were issued before the bin selection; the stream has been synchronised since)
  for (int64_t t = 0; t < S; ++t) n_gt2[(size_t)t] = h_gt2[(size_t)t];
  PoolBuf dorder, dperm;
  HIP_TRY(dorder.alloc((size_t)Sr * K * 4));
  HIP_TRY(dperm.alloc((size_t)Sr * 4));
  if (int rc = link.put(dorder.p, order_p.data(), (size_t)Sr * K * 4, st)) return rc;
  if (int rc = link.put(dperm.p, perm.data(), (size_t)Sr * 4, st)) return rc;
  // the column-major form of the chunk loop (k_rc_column) needs 16-bit tail counts: at most 65 535 bins; ED_REFCOHORT_ROWMAJOR (diagnostic) keeps the row-major kernels
  const bool columns = n <= 65535 && getenv("ED_REFCOHORT_ROWMAJOR") == nullptr;
  const int64_t np = (n + 63) / 64 * 64;
  PoolBuf dXT;
  if (columns) {
    HIP_TRY(dXT.alloc((size_t)S * np * 4));
    hipLaunchKernelGGL(k_rc_transpose, dim3((unsigned)((S + 31) / 32), (unsigned)((np + 31) / 32)), dim3(256), 0, st, dX.as<int32_t>(), n, S, np, dXT.as<int32_t>());
  }
  // ---- chunks of tests: K x T cumulative references, one batched fit, medians, RatioSd, expected Bayes factors ----
  const int64_t Tmax = std::max<int64_t>(1, std::min<int64_t>(Sr, ((int64_t)1 << 30) / std::max<int64_t>(n * K, 1)));   // cum <= 4 GiB
  std::vector<ed_refset_row> table((size_t)Sr * K);
  std::vector<char> fallback((size_t)Sr, 0);
  for (int64_t t0 = 0; t0 < Sr; t0 += Tmax) {           // (t0: a position of this call's layout, see perm)
    const int64_t T = std::min(Tmax, Sr - t0), R = (int64_t)K * T;
    PoolBuf dcum, dphi, dp, di32, dsize, dact, dbf, dpart2, dred2, dskip;
    HIP_TRY(dphi.alloc((size_t)R * 8));
    HIP_TRY(dp.alloc((size_t)R * 8));
    HIP_TRY(dskip.alloc((size_t)T * 4));                 // per test: the first prefix that is skipped
    HIP_TRY(di32.alloc((size_t)6 * R * 4));
    std::vector<int> skip_from((size_t)T, K);
    std::vector<double> phi((size_t)R), pbar((size_t)R), red2;
    std::vector<int32_t> med((size_t)6 * R);
    bool columns_done = false;
    if (columns) {
      // ---- column-major: one workgroup per cumulative reference (k_rc_column) ----
      for (int64_t j = 0; j < T; ++j) skip_from[(size_t)j] = stop[(size_t)(perm[(size_t)(t0 + j)] - tb)];
      PoolBuf dcumT, drsd, dflags;
      HIP_TRY(dcumT.alloc((size_t)R * np * 2));
      HIP_TRY(drsd.alloc((size_t)R * 8));
      HIP_TRY(dflags.alloc(32));
      if (int rc = link.put(dskip.p, skip_from.data(), (size_t)T * 4, st)) return rc;
      hipLaunchKernelGGL(k_rc_prefix_t, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, st, dXT.as<int32_t>(), dorder.as<int32_t>(),
                         dskip.as<int>(), n, np, t0, T, K, dcumT.as<uint16_t>());
      // Which geometry a column gets: its mean total (the column sums) x 2 for the spread of the bins' depths (bins above the 90 % quantile of the totals are
      // not selected, R/optimize_reference_set.R:84) against the small geometry's bins; what the small geometry cannot hold after all it hands on (`redo`).
      // A column beyond the large bins' reach by that measure leaves the chunk to the row-major kernels without trying.
      std::vector<int32_t> list_small, list_large;
      bool too_deep = false, may_hand_on = false;          // may_hand_on: a small-geometry column deep enough to run out of list (the large launch is issued beside it)
      double deepest = 0.0;
      for (int64_t j = 0; j < T; ++j) {
        double run = colsum[(size_t)perm[(size_t)(t0 + j)]];
        for (int k = 0; k < std::min(K, skip_from[(size_t)j]); ++k) {
          run += colsum[(size_t)order_p[(size_t)((t0 + j) * K + k)]];
          const double mean_n = run / (double)n;
          deepest = std::max(deepest, mean_n);
          if (2.0 * mean_n < (double)ColSmall::KN) { list_small.push_back((int32_t)((int64_t)k * T + j)); may_hand_on = may_hand_on || 1.25 * mean_n >= (double)ColSmall::KN; }
          else if (1.5 * mean_n < (double)ColBig::KN) list_large.push_back((int32_t)((int64_t)k * T + j));
          else too_deep = true;
        }
      }
      if (const char* ev = getenv("ED_REFCOHORT_GEOMETRY")) {      // (diagnostic / tests: every column through geometry 1 or 2 first; 0 = the row-major kernels)
        const int g = atoi(ev);
        too_deep = g == 0;
        if (g == 1) { list_small.insert(list_small.end(), list_large.begin(), list_large.end()); list_large.clear(); }
        if (g == 2) { list_large.insert(list_large.end(), list_small.begin(), list_small.end()); list_small.clear(); }
      }
      int flags[8] = {0};
      red2.resize((size_t)R);
      std::vector<int32_t> med2((size_t)2 * R);
      if (!too_deep) {
        PoolBuf dlist_s, dlist_l;
        HIP_TRY(dlist_s.alloc((size_t)R * 4));
        HIP_TRY(dlist_l.alloc((size_t)R * 4));
        const int n_small = (int)list_small.size(), n_large = (int)list_large.size();
        flags[6] = n_large;
        if (n_small) if (int rc = link.put(dlist_s.p, list_small.data(), (size_t)n_small * 4, st)) return rc;
        if (n_large) if (int rc = link.put(dlist_l.p, list_large.data(), (size_t)n_large * 4, st)) return rc;
        if (int rc = link.put(dflags.p, flags, 32, st)) return rc;
        // columns no list holds (prefixes no loop reaches) read as NaN / -1
        HIP_TRY(hipMemsetAsync(dphi.p, 0xff, (size_t)R * 8, st));
        HIP_TRY(hipMemsetAsync(dp.p, 0xff, (size_t)R * 8, st));
        HIP_TRY(hipMemsetAsync(drsd.p, 0xff, (size_t)R * 8, st));
        HIP_TRY(hipMemsetAsync(di32.p, 0xff, (size_t)2 * R * 4, st));
        if (n_small)
          hipLaunchKernelGGL(k_rc_column<ColSmall>, dim3((unsigned)n_small), dim3(ColSmall::NT), 0, st, dXT.as<int32_t>(), dcumT.as<uint16_t>(), dperm.as<int32_t>() + t0,
                             dskip.as<int>(), n, np, T, K, dphi.as<double>(), dp.as<double>(), drsd.as<double>(), di32.as<int32_t>(), dlist_s.as<int32_t>(), n_small,
                             dlist_l.as<int32_t>(), dflags.as<int>());
        int dev_now = 0, ncu = 256;
        (void)hipGetDevice(&dev_now);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev_now);
        auto launch_large = [&]() {
          hipLaunchKernelGGL(k_rc_column<ColBig>, dim3((unsigned)std::max(1, ncu)), dim3(ColBig::NT), 0, st, dXT.as<int32_t>(), dcumT.as<uint16_t>(), dperm.as<int32_t>() + t0,
                             dskip.as<int>(), n, np, T, K, dphi.as<double>(), dp.as<double>(), drsd.as<double>(), di32.as<int32_t>(), dlist_l.as<int32_t>(), -1,
                             (int32_t*)nullptr, dflags.as<int>());
        };
        // (a launch of one 1 024-thread workgroup per CU costs 0.1-0.15 ms even with an empty list: issued when a column is predicted for it or may be handed on)
        bool large_issued = n_large > 0 || may_hand_on || getenv("ED_REFCOHORT_GEOMETRY") != nullptr;
        if (large_issued) launch_large();
        if (int rc = link.get(flags, dflags.p, 32, st)) return rc;
        if (!large_issued) {                               // a hand-over nobody predicted: the large launch after all, and its results
          if (int rc = link.sync(st)) return rc;
          if (flags[6] > n_large) {
            large_issued = true;
            launch_large();
            if (int rc = link.get(flags, dflags.p, 32, st)) return rc;
          }
        }
        if (int rc = link.get(phi.data(), dphi.p, (size_t)R * 8, st)) return rc;
        if (int rc = link.get(pbar.data(), dp.p, (size_t)R * 8, st)) return rc;
        if (int rc = link.get(red2.data(), drsd.p, (size_t)R * 8, st)) return rc;
        if (int rc = link.get(med2.data(), di32.p, med2.size() * 4, st)) return rc;
        if (int rc = link.sync(st)) return rc;
        HIP_TRY(hipGetLastError());
        if (tick_on) fprintf(stderr, "[refcohort] columns: %d by the small geometry, %d by the large one (%d of them handed on), deepest prefix %.0f reads per bin; %d kept values beyond "
                                     "their bins (at most %d)%s, %d fits out of iterations, %d Newton iterations in all (at most %d)\n", n_small - (flags[6] - n_large), flags[6],
                             flags[6] - n_large, deepest, flags[3], flags[2], flags[0] ? "; a column beyond the large bins: row-major" : "", flags[1], flags[4], flags[5]);
      }
      columns_done = !too_deep && flags[0] == 0;
      g_rc_last_path[columns_done ? 0 : 1] += 1;
      g_rc_last_path[2] += flags[3];
      g_rc_last_path[3] = std::max<int64_t>(g_rc_last_path[3], flags[5]);
      g_rc_last_path[4] += columns_done ? flags[6] : 0;
      if (columns_done)
        for (int64_t r = 0; r < R; ++r) { med[(size_t)r] = med2[(size_t)r]; med[(size_t)(3 * R + r)] = med2[(size_t)(R + r)]; }   // (lo0 / lo1 of the bisection)
      tick(columns_done ? "columns: fit, medians, RatioSd" : "columns (left to the row-major kernels)");
    }
    if (!columns) g_rc_last_path[1] += 1;
    if (!columns_done) {
    // ---- row-major: the cumulative references as a matrix [bin][column], a kernel per step ----
    HIP_TRY(dcum.alloc((size_t)n * R * 4));
    HIP_TRY(dpart2.alloc((size_t)nchunk * kRsQ * R * 8));
    HIP_TRY(dred2.alloc((size_t)kRsQ * R * 8));
    hipLaunchKernelGGL(k_rc_prefix, dim3((unsigned)n), dim3(256), (size_t)S * 4, st, dX.as<int32_t>(), dorder.as<int32_t>(), n, S, t0, T, K,
                       dcum.as<int32_t>());
    PoolBuf dXp;                          // the chunk's test columns, in the chunk's order: column j = test perm[t0 + j]
    HIP_TRY(dXp.alloc((size_t)n * T * 4));
    hipLaunchKernelGGL(k_rc_gather_cols, dim3((unsigned)((T + 255) / 256), (unsigned)std::min<int64_t>(n, 1024)), dim3(256), 0, st, dX.as<int32_t>(),
                       dperm.as<int32_t>() + t0, n, S, T, dXp.as<int32_t>());
    tick("prefix sums");
    {
      FitWork* wp = nullptr;
      if (int rc = g_rc_scratch.fit_work(n, R, &wp)) return rc;
      FitWork& w = *wp;
      tick("fit workspace");
      const int rc = fit_columns(w, FitJob::cyclic_test(dXp.as<int32_t>(), T, dcum.as<int32_t>(), R, K, dskip.as<int>()).over(n, R).into(dphi.as<double>(), dp.as<double>()), st);
      if (int rc2 = link.sync(st)) return rc2;
      tick("batched fit");
      if (rc) return rc;
    }
    if (int rc = link.get(skip_from.data(), dskip.p, (size_t)T * 4, st)) return rc;
    if (int rc = link.get(phi.data(), dphi.p, (size_t)R * 8, st)) return rc;
    if (int rc = link.get(pbar.data(), dp.p, (size_t)R * 8, st)) return rc;
    // medians by bisection (two order statistics per column)
    const dim3 gcolw((unsigned)((R + kWave - 1) / kWave), (unsigned)nblk), gredw((unsigned)((R + kWave - 1) / kWave));
    const int64_t k0 = (n - 1) / 2, k1 = n / 2;
    {
      PoolBuf dpmax, dxmax;
      HIP_TRY(dpmax.alloc((size_t)nchunk * R * 4));
      HIP_TRY(dxmax.alloc((size_t)R * 4));
      if (int rc = refset_medians(dcum.as<int32_t>(), n, R, k0, k1, di32.as<int32_t>(), dpart2.as<double>(), dred2.as<double>(), dpmax.as<int32_t>(),
                                  dxmax.as<int32_t>(), dskip.as<int>(), K, T, st))
        return rc;
    }
    if (int rc = link.get(med.data(), di32.p, med.size() * 4, st)) return rc;
    hipLaunchKernelGGL(k_rc_ratiosd, gcolw, bcol, 0, st, dcum.as<int32_t>(), dXp.as<int32_t>(), T, (int64_t)0, T, n, R, dphi.as<double>(), dpart2.as<double>(), dskip.as<int>());
    if (int rc = reduce_to_host(dpart2, dred2, red2, R)) return rc;
    }
    tick("medians + RatioSd");
    // the loop's early exit per test (:130) and what is evaluated: column r = i * T + j
    std::vector<double> size_v((size_t)R);
    std::vector<int> active((size_t)R, 0);
    for (int64_t j = 0; j < T; ++j) {
      bool stopped = false;
      for (int i = 0; i < K; ++i) {
        const int64_t r = (int64_t)i * T + j;
        const double median = 0.5 * ((double)med[(size_t)r] + (double)med[(size_t)(3 * R + r)]);
        size_v[(size_t)r] = r_round(median);
        const int64_t tt = perm[(size_t)(t0 + j)] - tb;          // column j of the chunk is this test (index among this call's tests)
        ed_refset_row& o = table[(size_t)(tt * K + i)];
        o.ref_index = order[(size_t)(tt * K + i)]; o.selected = 0;
        o.correlation = corr_sorted[(size_t)(tt * K + i)];
        o.phi = phi[(size_t)r]; o.mean_p = pbar[(size_t)r]; o.median_depth = median; o.ratio_sd = red2[(size_t)r] / (double)n;
        o.expected_BF = std::nan("");
        if (!stopped && i >= skip_from[(size_t)j]) { fallback[(size_t)tt] = 1; stopped = true; }   // (never seen: the margin is 20 %)
        if (!stopped && i + 1 > 2 && pbar[(size_t)r] < 0.05) stopped = true;
        active[(size_t)r] = stopped ? 0 : 1;
      }
      if (!stopped && K < S - 1) fallback[(size_t)(perm[(size_t)(t0 + j)] - tb)] = 1;    // the R loop would run beyond the K prefixes formed here
    }
    HIP_TRY(dsize.alloc((size_t)R * 8)); HIP_TRY(dact.alloc((size_t)R * 4)); HIP_TRY(dbf.alloc((size_t)R * 8));
    if (int rc = link.put(dsize.p, size_v.data(), (size_t)R * 8, st)) return rc;
    if (int rc = link.put(dact.p, active.data(), (size_t)R * 4, st)) return rc;
    hipLaunchKernelGGL(k_rs_power_walk, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, dphi.as<double>(), dp.as<double>(), dsize.as<double>(),
                       dact.as<int>(), R, dbf.as<double>(), (const double*)nullptr);
    std::vector<double> bf((size_t)R);
    if (int rc = link.get(bf.data(), dbf.p, (size_t)R * 8, st)) return rc;
    if (int rc = link.sync(st)) return rc;
    HIP_TRY(hipGetLastError());
    tick("expected BF");
    for (int64_t j = 0; j < T; ++j)
      for (int i = 0; i < K; ++i) {
        const int64_t r = (int64_t)i * T + j;
        if (active[(size_t)r]) table[(size_t)(((int64_t)perm[(size_t)(t0 + j)] - tb) * K + i)].expected_BF = bf[(size_t)r];
      }
  }
  // ---- the choice per test (R/optimize_reference_set.R:143-145); tests beyond K or without coverage the slow way ----
  for (int64_t t = tb; t < te; ++t) {
    const int64_t tl = t - tb;
    ed_refset_row* tr = table.data() + tl * K;
    if (n_gt2[(size_t)t] < 5) {            // :57-61: too little coverage, the first candidate column
      n_chosen[tl] = 1;
      choice[tl * K] = (t == 0) ? 1 : 0;   // reference.counts[, 1] of the matrix without the test column
      continue;
    }
    if (fallback[(size_t)tl]) continue;
    int32_t nc = 0;
    if (int rc = ed_refset_finalize(tr, K, &nc)) return rc;
    n_chosen[tl] = nc;
    for (int k = 0; k < nc; ++k) choice[tl * K + k] = tr[k].ref_index;
  }
  // tests whose loop does not stop within K prefixes: the single-test entry on the matrix without the test's column (all S - 1
  // prefixes; slow, rare: it needs a cohort in which summing K samples still leaves the test above 5 % of the total)
  {
    DevBuf<void> dt, dr;
    std::vector<ed_refset_row> full;
    for (int64_t t = tb; t < te; ++t) {
      const int64_t tl = t - tb;
      if (!fallback[(size_t)tl]) continue;
      if (!dt.get()) { HIP_TRY(dt.alloc((size_t)E * 4)); HIP_TRY(dr.alloc((size_t)E * (S - 1) * 4)); full.resize((size_t)(S - 1)); }
      hipLaunchKernelGGL(k_rc_split_column, dim3((unsigned)((S + 255) / 256), (unsigned)std::min<int64_t>(E, 65535)), dim3(256), 0, st, d_counts, E, S, t,
                         dt.as<int32_t>(), dr.as<int32_t>());
      int32_t nc = 0;
      int64_t nsel = 0;
      if (int rc = ed_select_reference_set(dt.as<int32_t>(), dr.as<int32_t>(), E, S - 1, bin_length, n_bins_reduced, full.data(), &nc, &nsel, st)) return rc;
      if (nc > K) return ed_fail(ED_ERR_STATE, "ed_cohort_select_reference_sets: sample %lld chooses %d references, more than max_refs = %d: "
                                               "call again with a larger max_refs", (long long)t, (int)nc, K);
      n_chosen[tl] = nc;
      for (int k = 0; k < K; ++k) {
        ed_refset_row o = full[(size_t)k];
        o.ref_index += (o.ref_index >= t) ? 1 : 0;      // back to the cohort's columns
        table[(size_t)(tl * K + k)] = o;
        if (k < nc) choice[tl * K + k] = o.ref_index;
      }
    }
  }
  tick("choice (+ fallbacks)");
  if (rows) std::memcpy(rows, table.data(), table.size() * sizeof(ed_refset_row));
  PoolBuf dref_tmp;          // sample-major outputs of a geometry k_rc_aggregate_sm does not take: the [n_bins][n_tests] form first, then transposed
  bool sm_by_transposition = false;
  if (d_ref_sm_out) {       // sample-major aggregate references (+ the transposed counts): k_rc_aggregate_sm
    // rows per tile: the largest of 32 / 16 / 8 whose tile fits LDS next to the lists
    int R = 0;
    size_t lds = 0;
    for (int cand : {32, 16, 8}) {
      const size_t need = (size_t)S * (cand + 1) * 4 + (size_t)Sr * ((K + 7) & ~7) * 2 + 16;
      if (need <= 156 * 1024) { R = cand; lds = need; break; }
    }
    if (R == 0 || S > 65534) {
      sm_by_transposition = true;
      if (!d_ref_out) { HIP_TRY(dref_tmp.alloc((size_t)E * Sr * 4)); d_ref_out = dref_tmp.as<int32_t>(); }
    } else {
      PoolBuf dchoice;
      HIP_TRY(dchoice.alloc((size_t)Sr * K * 4));
      if (int rc = link.put(dchoice.p, choice, (size_t)Sr * K * 4, st)) return rc;
      if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)k_rc_aggregate_sm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      int ncu = 256;
      { hipDeviceProp_t prop; int dev = 0; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount; }
      const int64_t ntile = (E + R - 1) / R;
      hipLaunchKernelGGL(k_rc_aggregate_sm, dim3((unsigned)std::min<int64_t>(ntile, ncu)), dim3(kAggSmThreads), lds, st, d_counts, dchoice.as<int32_t>(),
                         E, S, K, R, d_ref_sm_out, Sr, d_counts_sm_out);
      HIP_TRY(hipGetLastError());
      if (int rc = link.sync(st)) return rc;
    }
  }
  if (d_ref_out) {
    PoolBuf dchoice, dnc;
    HIP_TRY(dchoice.alloc((size_t)Sr * K * 4)); HIP_TRY(dnc.alloc((size_t)Sr * 4));
    if (int rc = link.put(dchoice.p, choice, (size_t)Sr * K * 4, st)) return rc;
    if (int rc = link.put(dnc.p, n_chosen, (size_t)Sr * 4, st)) return rc;
    {
      const int rows = (int)std::max<int64_t>(1, std::min<int64_t>(kAggRowsMax, 16384 / S));   // tile = rows x S x 4 B <= 64 KB
      const int64_t nwg_y = std::max<int64_t>(1, std::min<int64_t>((E + rows - 1) / rows, 2048 / ((Sr + 255) / 256) + 1));
      const int64_t rows_per_wg = ((E + nwg_y - 1) / nwg_y + rows - 1) / rows * rows;
      const size_t lds = (size_t)rows * S * 4;
      if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)k_rc_aggregate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_rc_aggregate, dim3((unsigned)((Sr + 255) / 256), (unsigned)((E + rows_per_wg - 1) / rows_per_wg)), dim3(256), lds, st, d_counts,
                         dchoice.as<int32_t>(), dnc.as<int32_t>(), E, S, K, rows, rows_per_wg, d_ref_out, Sr);
    }
    HIP_TRY(hipGetLastError());
    if (sm_by_transposition) {
      hipLaunchKernelGGL(k_tab_rows_to_cols, dim3((unsigned)((E + 63) / 64), (unsigned)((Sr + 63) / 64)), dim3(256), 0, st, d_ref_out, E, Sr, d_ref_sm_out);
      if (d_counts_sm_out)
        hipLaunchKernelGGL(k_tab_rows_to_cols, dim3((unsigned)((E + 63) / 64), (unsigned)((S + 63) / 64)), dim3(256), 0, st, d_counts, E, S, d_counts_sm_out);
      HIP_TRY(hipGetLastError());
    }
    if (int rc = link.sync(st)) return rc;
  }
  tick("aggregate references");
  return ED_OK;
}

ED_EXPORT int ed_cohort_select_reference_sets_range(const int32_t* d_counts, int64_t n_bins, int64_t n_samples, const double* bin_length,
                                                    int64_t n_bins_reduced, int32_t max_refs, int64_t test_begin, int64_t test_end,
                                                    int32_t* n_chosen, int32_t* choice, ed_refset_row* rows, double* correlations,
                                                    int32_t* d_ref_out, int64_t* n_selected_bins, void* stream_)
try {
  return refcohort_impl(d_counts, n_bins, n_samples, bin_length, n_bins_reduced, max_refs, test_begin, test_end, n_chosen, choice, rows, correlations,
                        d_ref_out, n_selected_bins, stream_, nullptr, nullptr);
}
ED_CATCH("ed_cohort_select_reference_sets_range")

// ... with the aggregate references written sample-major, d_ref_sm_out [n_tests][n_bins], and optionally the count matrix transposed
// alongside, d_counts_sm_out [n_samples][n_bins]: what a cohort with option counts_layout = 1 (emit mode 2) takes as they are.
ED_EXPORT int ed_cohort_select_reference_sets_sm(const int32_t* d_counts, int64_t n_bins, int64_t n_samples, const double* bin_length,
                                                 int64_t n_bins_reduced, int32_t max_refs, int64_t test_begin, int64_t test_end,
                                                 int32_t* n_chosen, int32_t* choice, ed_refset_row* rows, double* correlations,
                                                 int32_t* d_ref_sm_out, int32_t* d_counts_sm_out, int64_t* n_selected_bins, void* stream_)
try {
  if (!d_ref_sm_out) return ed_fail(ED_ERR_INVALID, "ed_cohort_select_reference_sets_sm: NULL output");
  return refcohort_impl(d_counts, n_bins, n_samples, bin_length, n_bins_reduced, max_refs, test_begin, test_end, n_chosen, choice, rows, correlations,
                        nullptr, n_selected_bins, stream_, d_ref_sm_out, d_counts_sm_out);
}
ED_CATCH("ed_cohort_select_reference_sets_sm")

ED_EXPORT int ed_cohort_select_reference_sets(const int32_t* d_counts, int64_t n_bins, int64_t n_samples, const double* bin_length,
                                              int64_t n_bins_reduced, int32_t max_refs, int32_t* n_chosen, int32_t* choice,
                                              ed_refset_row* rows, double* correlations, int32_t* d_ref_out, int64_t* n_selected_bins,
                                              void* stream_)
try {
  return ed_cohort_select_reference_sets_range(d_counts, n_bins, n_samples, bin_length, n_bins_reduced, max_refs, 0, n_samples, n_chosen, choice, rows,
                                               correlations, d_ref_out, n_selected_bins, stream_);
}
ED_CATCH("ed_cohort_select_reference_sets")

// how the chunks of the last ed_cohort_select_reference_sets* call of this process were served: out = {chunks by the column-major kernel, chunks by the
// row-major kernels, columns that kept counts beyond their bins as values, the most Newton iterations a column took, columns served by the large geometry}
ED_EXPORT int ed_refcohort_last_path(int64_t out[5])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> scratch_lock(g_rc_scratch.mu);
  for (int q = 0; q < 5; ++q) out[q] = g_rc_last_path[q];
  return ED_OK;
}
ED_CATCH("ed_refcohort_last_path")

// gives the scratch kept between calls of ed_cohort_select_reference_sets back to the device
ED_EXPORT int ed_release_scratch(void)
try {
  std::lock_guard<std::mutex> scratch_lock(g_rc_scratch.mu);
  g_rc_scratch.release_all();
  g_rc_scratch.device = -1;
  return ED_OK;
}
ED_CATCH("ed_release_scratch")

ED_EXPORT void ed_live_allocations(int64_t* n, int64_t* bytes)
{
  if (n) *n = edown::g_live_n.load(std::memory_order_relaxed);
  if (bytes) *bytes = edown::g_live_bytes.load(std::memory_order_relaxed);
}

// The same on host data in R's layout: counts = the n_bins x n_samples integer matrix, column-major; reference_out (optional) the
// aggregate reference in that layout.  What the R-level wrapper ed_cohort_reference_sets (shim/edcore_shim.c) calls.
ED_EXPORT int ed_cohort_select_reference_sets_host(const int32_t* counts_colmajor, int64_t n_bins, int64_t n_samples, const double* bin_length,
                                                   int64_t n_bins_reduced, int32_t max_refs, int32_t* n_chosen, int32_t* choice,
                                                   ed_refset_row* rows, double* correlations, int32_t* reference_out_colmajor,
                                                   int64_t* n_selected_bins)
try {
  if (!counts_colmajor || n_bins <= 0 || n_samples < 2) return ed_fail(ED_ERR_INVALID, "ed_cohort_select_reference_sets_host: bad arguments");
  if (int rc = require_device()) return rc;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int64_t E = n_bins, S = n_samples;
  struct Work { DevBuf<void> c, raw, ref; HostFeed f; } k;      // (the feed goes before the buffers)
  if (int rc = k.f.open(dev)) return rc;
  HIP_TRY(k.c.alloc((size_t)E * S * 4)); HIP_TRY(k.raw.alloc((size_t)E * S * 4));
  if (reference_out_colmajor) HIP_TRY(k.ref.alloc((size_t)E * S * 4));
  if (int rc = upload_counts(k.f.g.get(), k.f.s, counts_colmajor, E, S, 1, 4, S, k.raw.get(), k.c.as<int32_t>())) return rc;
  // R's column-major n_bins x n_samples matrix IS the sample-major form: the aggregate references are written that way directly
  if (int rc = refcohort_impl(k.c.as<int32_t>(), E, S, bin_length, n_bins_reduced, max_refs, 0, S, n_chosen, choice, rows, correlations, nullptr,
                              n_selected_bins, k.f.s, reference_out_colmajor ? k.ref.as<int32_t>() : nullptr, nullptr))
    return rc;
  if (reference_out_colmajor) { if (int rc = ed_d2h(reference_out_colmajor, k.ref.get(), (size_t)E * S * 4, k.f.s)) return rc; }
  return ED_OK;
}
ED_CATCH("ed_cohort_select_reference_sets_host")
