// edpca.inc -- correct.counts.using.PCA (R/PCA_for_read_count.R:41-78) for a whole cohort on the device (included at the end of edcore.hip).
//
// With C the E x S count matrix (counts[E][S], int32, the layout the reference-set stage takes):
//   :50     rs[e] = rowSums(C)[e] / 1000                     one value per EXON
//   :51     N[e][s] = C[e][s] / max(1, rs[s])                the reference indexes the per-exon vector by the SAMPLE number (its quirk; S <= E)
//   :55     centre[e] = mean_s N[e][s]
//   :56     good[e] = sd_s(N[e][.]) > 2                      (n - 1 denominator)
//   :58     Z = N - centre
//   :63-65  prcomp of the columns good & !mask of t(Z): U_k = the top nPCs eigenvectors of G = sum_{e selected} Z[e][.] Z[e][.]^T  (S x S)
//   :68-74  the scores regressed out of ALL exons: R[e][.] = (I - U_k U_k^T) Z[e][.]
//   :75     out[e][s] = round(max(0, rs[e] * (R[e][s] + centre[e])))        round = half-even = rint
// The three vectors are arguments of the C entry: div[s] (NULL: max(1, rs[s])), exon_mul[e] (NULL: rs[e]), sample_mul[s] (NULL: 1).
//
// Stages (no E x S array of doubles exists at any time; temporaries are O(E + S^2 + slices S^2)):
//   1  k_pca_rowsum / k_pca_div / k_pca_rowstats / k_pca_compact   a wave per exon row; the ordered list of selected exons
//   2  k_pca_gram + k_pca_gram_sum     G with v_mfma_f64_16x16x4_f64, z formed on the fly from the int32 counts, rows staged through LDS
//   3  k_pca_*  (dots, jacobi, chol, rmul, rotate, colnorm2)         block subspace iteration with Rayleigh-Ritz; the b x b Ritz problem by cyclic Jacobi
//   4  k_pca_residual                  one pass over the counts: z, t = U_k^T z, r = z - U_k t, the rounding rule, int32 out

namespace {

constexpr int kPcaTile = 128;       // a workgroup owns a 128 x 128 tile of G: 4 waves, 64 x 64 each = 4 x 4 MFMA blocks, 128 accumulator registers a lane
constexpr int kPcaChunk = 16;       // selected rows staged through LDS at a time (4 MFMA k-steps)
constexpr int kPcaLd = 144;         // LDS row stride in doubles: 288 dwords = 32 mod 64, so the four k-rows a fragment read touches fall on disjoint bank halves
constexpr int kPcaGramSlices = 14;  // the selected rows are cut into this many slices: 36 lower-triangle tiles (S = 1024) x 14 = 504 workgroups <= 256 CUs x 2 resident
constexpr int kPcaMaxPcs = 64;
constexpr int kPcaMaxBlock = 128;   // b = min(S, max(2k, k + 8)) <= 128
constexpr int64_t kPcaMaxSamples = 32768;

__device__ __forceinline__ double pca_wave_sum(double v)
{
  // xor butterfly: a fixed order, and every lane ends with the same bits (a + b == b + a)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// 256 threads: the sum of v over the block, the same bits in every thread and on every run
__device__ __forceinline__ double pca_block_sum(double v, double* sh /* [4] */)
{
  v = pca_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// rs[e] = rowSums(counts)[e] / 1000 (:50); the integer sum is exact.  A wave per row.
__global__ void __launch_bounds__(256)
k_pca_rowsum(const int32_t* __restrict__ counts, int64_t E, int64_t S, double* __restrict__ rs)
{
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const int32_t* __restrict__ row = counts + e * S;
  long long acc = 0;
  for (int64_t s = lane; s < S; s += 64) acc += row[s];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if (lane == 0) rs[e] = (double)acc / 1000.0;
}

// div[s] = max(1, rs[s]) (:51): the per-exon vector indexed by the sample number
__global__ void __launch_bounds__(256)
k_pca_div(const double* __restrict__ rs, int64_t S, double* __restrict__ div)
{
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < S) div[s] = rs[s] > 1.0 ? rs[s] : 1.0;
}

// centre[e] = mean_s N[e][s] (:55), sd two-pass within the row (:56); flag[e] = sd > sd_min and not masked.  A wave per row.
__global__ void __launch_bounds__(256)
k_pca_rowstats(const int32_t* __restrict__ counts, int64_t E, int64_t S, const double* __restrict__ div, const uint8_t* __restrict__ mask, double sd_min,
               double* __restrict__ centre, uint8_t* __restrict__ flag)
{
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const int32_t* __restrict__ row = counts + e * S;
  double a = 0.0;
  for (int64_t s = lane; s < S; s += 64) a += (double)row[s] / div[s];
  const double mean = pca_wave_sum(a) / (double)S;
  double q = 0.0;
  for (int64_t s = lane; s < S; s += 64) {
    const double d = (double)row[s] / div[s] - mean;
    q += d * d;
  }
  const double sd = __builtin_sqrt(pca_wave_sum(q) / (double)(S - 1));
  if (lane == 0) {
    centre[e] = mean;
    flag[e] = (uint8_t)((sd > sd_min) && !(mask && mask[e]));
  }
}

// the selected exons in increasing order: one workgroup, each thread a contiguous range, an exclusive scan of the counts
__global__ void __launch_bounds__(1024)
k_pca_compact(const uint8_t* __restrict__ flag, int64_t E, int32_t* __restrict__ sel, int64_t* __restrict__ n_out)
{
  __shared__ int64_t sc[1024];
  const int t = threadIdx.x;
  const int64_t per = (E + 1023) / 1024, lo = (int64_t)t * per < E ? (int64_t)t * per : E, hi = lo + per < E ? lo + per : E;
  int64_t c = 0;
  for (int64_t e = lo; e < hi; ++e) c += flag[e];
  sc[t] = c;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t add = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  int64_t w = sc[t] - c;
  for (int64_t e = lo; e < hi; ++e) if (flag[e]) sel[w++] = (int32_t)e;
  if (t == 1023) *n_out = sc[1023];
}

// G = sum over the selected exons of z z^T, z[s] = counts[e][s] / div[s] - centre[e] formed on the fly (no Z in memory).
// A workgroup (256 threads) owns a 128 x 128 tile of the lower triangle of G and one slice of the selected rows.  Sixteen rows at a time are
// staged through LDS (both column ranges of the tile, as doubles) and every wave reads its fragments from there: a count is read from memory and
// turned into z once per workgroup tile, not once per MFMA block.  Fragment layout as above k_rc_gram: A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15], D: col = lane & 15, row = (lane >> 4) + 4 * reg.  Columns >= S and rows >= n are zeros.
// part [slices][Sp][Sp]; k_pca_gram_sum adds the slices in a fixed order (no floating-point atomics).
__global__ void __launch_bounds__(256)
k_pca_gram(const int32_t* __restrict__ counts, const int32_t* __restrict__ sel, int64_t n, int64_t S, const double* __restrict__ div,
           const double* __restrict__ centre, int64_t Sp, double* __restrict__ part)
{
  __shared__ double zs[2][kPcaChunk][kPcaLd];
  int ta = 0;
  {
    const int L = blockIdx.x;
    while ((ta + 1) * (ta + 2) / 2 <= L) ++ta;
  }
  const int tb = (int)blockIdx.x - ta * (ta + 1) / 2;        // tb <= ta: the lower triangle of tiles
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wa = w >> 1, wb = w & 1;
  const int side = t >> 7, col = t & 127;
  const int64_t gcol = (int64_t)(side ? tb : ta) * kPcaTile + col;
  const bool valid = gcol < S;
  const double dv = valid ? div[gcol] : 1.0;
  const int64_t chunks = (n + kPcaChunk - 1) / kPcaChunk, per = (chunks + kPcaGramSlices - 1) / kPcaGramSlices;
  const int64_t c0 = (int64_t)blockIdx.y * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  v4d acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4d{0, 0, 0, 0};
  int32_t pre[kPcaChunk];
  double cen[kPcaChunk];
  auto fetch = [&](int64_t c) {
#pragma unroll
    for (int r = 0; r < kPcaChunk; ++r) {
      const int64_t row = c * kPcaChunk + r;
      pre[r] = 0; cen[r] = 0.0;
      if (row < n && valid) {
        const int64_t e = sel[row];
        pre[r] = counts[e * S + gcol];
        cen[r] = centre[e];
      }
    }
  };
  if (c0 < c1) fetch(c0);
  for (int64_t c = c0; c < c1; ++c) {
#pragma unroll
    for (int r = 0; r < kPcaChunk; ++r) zs[side][r][col] = (double)pre[r] / dv - cen[r];
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
    const int64_t left = n - c * kPcaChunk;
    const int ksteps = left >= kPcaChunk ? kPcaChunk / 4 : (int)((left + 3) / 4);
    for (int kk = 0; kk < ksteps; ++kk) {
      const int k = kk * 4 + (lane >> 4);
      double fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa[i] = zs[0][k][wa * 64 + 16 * i + (lane & 15)];
        fb[i] = zs[1][k][wb * 64 + 16 * i + (lane & 15)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  double* __restrict__ out = part + (int64_t)blockIdx.y * Sp * Sp;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ra = (int64_t)ta * kPcaTile + wa * 64 + 16 * i + (lane >> 4) + 4 * r;
        const int64_t cb = (int64_t)tb * kPcaTile + wb * 64 + 16 * j + (lane & 15);
        out[ra * Sp + cb] = acc[i][j][r];
      }
}

// G[a][b] (S x S, unpadded, both triangles) = the slices' partial sums in slice order
__global__ void __launch_bounds__(256)
k_pca_gram_sum(const double* __restrict__ part, int64_t Sp, int64_t S, double* __restrict__ G)
{
  const int64_t a = blockIdx.y, b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= S) return;
  const int64_t hi = a > b ? a : b, lo = a > b ? b : a;
  double s = 0.0;
  for (int z = 0; z < kPcaGramSlices; ++z) s += part[(int64_t)z * Sp * Sp + hi * Sp + lo];
  G[a * S + b] = s;
}

// ---- stage 3: the top-k eigenvectors of G by block subspace iteration with Rayleigh-Ritz ----
// matrices of the iteration are row-major [S][b]

__device__ __forceinline__ double pca_hash_unit(uint64_t x)
{
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  x ^= x >> 31;
  return (double)(x >> 11) * 0x1p-52 - 1.0;      // (-1, 1)
}
__global__ void __launch_bounds__(256)
k_pca_init(int64_t nel, double* __restrict__ Q)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nel) Q[i] = pca_hash_unit((uint64_t)i);
}

// out[i * ldo + j] = sum_t P[i * pi + t * pt] * Q[t * qt + j * qj], t < len; a workgroup per entry, a fixed summation order
__global__ void __launch_bounds__(256)
k_pca_dots(const double* __restrict__ P, int64_t pi, int64_t pt, const double* __restrict__ Q, int64_t qt, int64_t qj, int64_t len,
           double* __restrict__ out, int64_t ldo)
{
  __shared__ double sh[4];
  const int64_t i = blockIdx.y, j = blockIdx.x;
  double a = 0.0;
  for (int64_t t = threadIdx.x; t < len; t += 256) a += P[i * pi + t * pt] * Q[t * qt + j * qj];
  a = pca_block_sum(a, sh);
  if (threadIdx.x == 0) out[i * ldo + j] = a;
}

// out[s][j] = sum_i A[s][i] M[i][j]  (row-local right multiplication by a b x b matrix)
__global__ void __launch_bounds__(256)
k_pca_rmul(const double* __restrict__ A, const double* __restrict__ M, int64_t S, int b, double* __restrict__ out)
{
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * b) return;
  const int64_t s = idx / b;
  const int j = (int)(idx - s * b);
  double a = 0.0;
  for (int i = 0; i < b; ++i) a += A[s * b + i] * M[(int64_t)i * b + j];
  out[idx] = a;
}

// the Ritz vectors X = Q W, their images Y = Z W (Z = G Q), and the residuals Rr = Y - X diag(theta)
__global__ void __launch_bounds__(256)
k_pca_rotate(const double* __restrict__ Q, const double* __restrict__ Z, const double* __restrict__ W, const double* __restrict__ theta, int64_t S, int b,
             double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Rr)
{
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * b) return;
  const int64_t s = idx / b;
  const int j = (int)(idx - s * b);
  double x = 0.0, y = 0.0;
  for (int i = 0; i < b; ++i) {
    const double wij = W[(int64_t)i * b + j];
    x += Q[s * b + i] * wij;
    y += Z[s * b + i] * wij;
  }
  X[idx] = x; Y[idx] = y; Rr[idx] = y - theta[j] * x;
}

// out[j] = sum_s A[s][j]^2, j = blockIdx.x
__global__ void __launch_bounds__(256)
k_pca_colnorm2(const double* __restrict__ A, int64_t S, int b, double* __restrict__ out)
{
  __shared__ double sh[4];
  const int j = blockIdx.x;
  double a = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += 256) { const double v = A[s * b + j]; a += v * v; }
  a = pca_block_sum(a, sh);
  if (threadIdx.x == 0) out[j] = a;
}

// Eigen-decomposition of the symmetric b x b matrix H (b <= 128) by cyclic Jacobi, one workgroup of 128 threads: thread t owns row / column t of
// the rotation's updates and row t of the accumulated rotations.  H lives in LDS; the rotations too when both fit (w_in_lds), else in Wtmp (global;
// a thread only ever touches its own row of it).  Out: theta[b] in decreasing order, Wout[i][rank] the eigenvectors in that order.
__global__ void __launch_bounds__(128)
k_pca_jacobi(const double* __restrict__ Hin, int b, int w_in_lds, double* __restrict__ Wtmp, double* __restrict__ Wout, double* __restrict__ theta)
{
  extern __shared__ double pca_lds[];
  double* H = pca_lds;
  double* W = w_in_lds ? pca_lds + b * b : Wtmp;
  const int t = threadIdx.x;
  for (int idx = t; idx < b * b; idx += 128) {
    const int i = idx / b, j = idx - i * b;
    H[idx] = 0.5 * (Hin[i * b + j] + Hin[j * b + i]);
  }
  if (t < b) for (int j = 0; j < b; ++j) W[t * b + j] = (j == t) ? 1.0 : 0.0;
  __syncthreads();
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool any = false;                       // the same in every thread: all of them read the same three entries
    for (int p = 0; p < b - 1; ++p)
      for (int q = p + 1; q < b; ++q) {
        const double hpq = H[p * b + q], hpp = H[p * b + p], hqq = H[q * b + q];
        const double small = 0x1p-70 * __builtin_sqrt(__builtin_fabs(hpp) * __builtin_fabs(hqq));
        if (!(__builtin_fabs(hpq) > small) || !(__builtin_fabs(hpq) > 1e-300)) continue;
        any = true;
        const double tau = (hqq - hpp) / (2.0 * hpq);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(tau) + __builtin_sqrt(1.0 + tau * tau));
        const double c = 1.0 / __builtin_sqrt(1.0 + tt * tt), s = tt * c;
        __syncthreads();                    // every thread has read (p,p), (q,q), (p,q)
        if (t < b) {
          if (t != p && t != q) {
            const double htp = H[t * b + p], htq = H[t * b + q];
            const double ntp = c * htp - s * htq, ntq = s * htp + c * htq;
            H[t * b + p] = ntp; H[p * b + t] = ntp; H[t * b + q] = ntq; H[q * b + t] = ntq;
          } else if (t == p) {
            H[p * b + p] = hpp - tt * hpq; H[q * b + q] = hqq + tt * hpq; H[p * b + q] = 0.0; H[q * b + p] = 0.0;
          }
          const double wp = W[t * b + p], wq = W[t * b + q];
          W[t * b + p] = c * wp - s * wq; W[t * b + q] = s * wp + c * wq;
        }
        __syncthreads();
      }
    if (!any) break;
  }
  __threadfence();                          // (rotations kept in global memory: the other threads' rows are read below)
  __syncthreads();
  if (t < b) {
    const double mine = H[t * b + t];
    int rank = 0;
    for (int j = 0; j < b; ++j) {
      const double o = H[j * b + j];
      rank += (o > mine) || (o == mine && j < t);
    }
    theta[rank] = mine;
    for (int i = 0; i < b; ++i) Wout[i * b + rank] = W[i * b + t];
  }
}

// M = R^T R (Cholesky, R upper triangular); out Rinv = R^-1, so that Y Rinv has orthonormal columns when M = Y^T Y.  One workgroup of 128 threads;
// thread t owns row t of the factor and row t of Rinv.  *bad = 1 when a pivot is not positive (the basis lost rank).
__global__ void __launch_bounds__(128)
k_pca_chol(const double* __restrict__ M, int b, int x_in_lds, double* __restrict__ Rinv, int* __restrict__ bad)
{
  extern __shared__ double pca_lds[];
  double* L = pca_lds;
  double* X = x_in_lds ? pca_lds + b * b : Rinv;
  const int t = threadIdx.x;
  for (int idx = t; idx < b * b; idx += 128) {
    const int i = idx / b, j = idx - i * b;
    L[idx] = 0.5 * (M[i * b + j] + M[j * b + i]);
  }
  __syncthreads();
  for (int j = 0; j < b; ++j) {
    const double d2 = L[j * b + j];
    if (!(d2 > 0.0) || !(d2 < 1e300)) {       // the same decision in every thread
      if (t == 0) *bad = 1;
      for (int idx = t; idx < b * b; idx += 128) Rinv[idx] = (idx / b == idx % b) ? 1.0 : 0.0;
      return;
    }
    const double d = __builtin_sqrt(d2);
    __syncthreads();
    if (t == j) L[j * b + j] = d;
    if (t > j && t < b) L[t * b + j] = L[t * b + j] / d;
    __syncthreads();
    if (t > j && t < b)
      for (int c = j + 1; c <= t; ++c) L[t * b + c] -= L[t * b + j] * L[c * b + j];
    __syncthreads();
  }
  // column t of L^-1 by forward substitution = row t of R^-1 (R = L^T)
  if (t < b) {
    for (int r = 0; r < t; ++r) X[t * b + r] = 0.0;
    X[t * b + t] = 1.0 / L[t * b + t];
    for (int r = t + 1; r < b; ++r) {
      double a = 0.0;
      for (int m = t; m < r; ++m) a += L[r * b + m] * X[t * b + m];
      X[t * b + r] = -a / L[r * b + r];
    }
    if (x_in_lds) for (int r = 0; r < b; ++r) Rinv[t * b + r] = X[t * b + r];
  }
}

// ---- stage 4: out[e][s] = rint(max(0, exon_mul[e] * sample_mul[s] * (r + centre[e]))), r = z - U_k (U_k^T z); every exon, selected or not ----
// A wave per exon row.  U [S][ldu] (the first k columns); its copy [S][k] sits in LDS when u_in_lds, else it is read through L2.
__global__ void __launch_bounds__(256)
k_pca_residual(const int32_t* __restrict__ counts, int64_t E, int64_t S, const double* __restrict__ div, const double* __restrict__ centre,
               const double* __restrict__ emul, const double* __restrict__ smul, const double* __restrict__ U, int ldu, int k, int u_in_lds,
               int32_t* __restrict__ out)
{
  extern __shared__ double pca_lds[];
  const double* Uk = U;
  int ld = ldu;
  if (u_in_lds) {
    for (int64_t idx = threadIdx.x; idx < S * k; idx += 256) pca_lds[idx] = U[(idx / k) * ldu + idx % k];
    __syncthreads();
    Uk = pca_lds; ld = k;
  }
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  const int64_t Sr = (S + 63) / 64 * 64;
  for (int64_t e = wave; e < E; e += nwaves) {
    const int32_t* __restrict__ row = counts + e * S;
    const double cen = centre[e], em = emul[e];
    double tmine = 0.0;                      // lane j keeps t_j = sum_s U[s][j] z[s]
    for (int j = 0; j < k; ++j) {
      double a = 0.0;
      for (int64_t s = lane; s < S; s += 64) a += Uk[s * ld + j] * ((double)row[s] / div[s] - cen);
      a = pca_wave_sum(a);
      if (lane == j) tmine = a;
    }
    for (int64_t s0 = 0; s0 < Sr; s0 += 64) {
      const int64_t s = s0 + lane;
      const bool in = s < S;
      const double z = in ? (double)row[s] / div[s] - cen : 0.0;
      double proj = 0.0;
      for (int j = 0; j < k; ++j) {
        const double tj = __shfl(tmine, j, 64);
        if (in) proj += Uk[s * ld + j] * tj;
      }
      if (in) {
        const double m = smul ? em * smul[s] : em;
        double v = m * ((z - proj) + cen);
        v = v > 0.0 ? v : 0.0;               // pmax(0, .): a NaN becomes 0
        v = v < 2147483647.0 ? v : 2147483647.0;
        out[e * S + s] = (int32_t)__builtin_rint(v);
      }
    }
  }
}

// what ed_pca_last_info reports (under the mutex): see include/exomedepth_amd.h
std::mutex g_pca_mu;
double g_pca_info[ED_PCA_INFO_N] = {0};
std::vector<double> g_pca_basis;        // the last call's U_k, [S][k]
int64_t g_pca_basis_S = 0, g_pca_basis_k = 0;

struct PcaStage12 {
  DevBuf<void> rs, div, centre, flag, mask, sel, nsel, part, G;
  int64_t n = 0, Sp = 0;
};

}  // namespace

static int pca_check_args(const char* who, const void* d_counts, int64_t E, int64_t S, const double* sample_div)
{
  if (!d_counts) return ed_fail(ED_ERR_INVALID, "%s: NULL count matrix", who);
  if (E <= 0 || S < 2) return ed_fail(ED_ERR_INVALID, "%s: %lld exons x %lld samples (at least 1 exon and 2 samples)", who, (long long)E, (long long)S);
  if (S > kPcaMaxSamples) return ed_fail(ED_ERR_INVALID, "%s: %lld samples, at most %lld per call", who, (long long)S, (long long)kPcaMaxSamples);
  if (E > 2147483647LL) return ed_fail(ED_ERR_INVALID, "%s: %lld exons, at most 2^31 - 1", who, (long long)E);
  if (!sample_div && S > E)
    return ed_fail(ED_ERR_INVALID, "%s: %lld samples but %lld exons: the reference's divisor max(1, rowSums[s] / 1000) indexes the per-exon sums by the "
                   "sample number and needs n_samples <= n_exons (or pass sample_div)", who, (long long)S, (long long)E);
  if (sample_div)
    for (int64_t s = 0; s < S; ++s)
      if (!(sample_div[s] > 0.0) || !std::isfinite(sample_div[s]))
        return ed_fail(ED_ERR_INVALID, "%s: sample_div[%lld] = %g: the divisors must be finite and positive", who, (long long)s, sample_div[s]);
  return ED_OK;
}

// stages 1 and 2 on stream st: row statistics, the selected list, G.  ev (optional): events recorded at the start, after stage 1, after stage 2.
static int pca_stage12(const char* who, const int32_t* d_counts, int64_t E, int64_t S, const uint8_t* mask_exons, const double* sample_div, double sd_min,
                       hipStream_t st, PcaStage12& w, const Event* ev)
{
  HIP_TRY(w.rs.alloc((size_t)E * 8)); HIP_TRY(w.div.alloc((size_t)S * 8)); HIP_TRY(w.centre.alloc((size_t)E * 8));
  HIP_TRY(w.flag.alloc((size_t)E)); HIP_TRY(w.sel.alloc((size_t)E * 4)); HIP_TRY(w.nsel.alloc(8));
  if (mask_exons) {
    HIP_TRY(w.mask.alloc((size_t)E));
    HIP_TRY(hipMemcpyAsync(w.mask.get(), mask_exons, (size_t)E, hipMemcpyHostToDevice, st));
  }
  if (ev) HIP_TRY(hipEventRecord(ev[0], st));
  const unsigned row_blocks = (unsigned)((E + 3) / 4);
  hipLaunchKernelGGL(k_pca_rowsum, dim3(row_blocks), dim3(256), 0, st, d_counts, E, S, w.rs.as<double>());
  if (sample_div) HIP_TRY(hipMemcpyAsync(w.div.get(), sample_div, (size_t)S * 8, hipMemcpyHostToDevice, st));
  else hipLaunchKernelGGL(k_pca_div, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, w.rs.as<double>(), S, w.div.as<double>());
  hipLaunchKernelGGL(k_pca_rowstats, dim3(row_blocks), dim3(256), 0, st, d_counts, E, S, w.div.as<double>(), mask_exons ? w.mask.as<uint8_t>() : nullptr,
                     sd_min, w.centre.as<double>(), w.flag.as<uint8_t>());
  hipLaunchKernelGGL(k_pca_compact, dim3(1), dim3(1024), 0, st, w.flag.as<uint8_t>(), E, w.sel.as<int32_t>(), w.nsel.as<int64_t>());
  HIP_TRY(hipGetLastError());
  if (int rc = ed_d2h(&w.n, w.nsel.get(), 8, st)) return rc;
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  if (w.n < 1) return ed_fail(ED_ERR_INVALID, "%s: no exon has a standard deviation above sd_min = %g%s", who, sd_min, mask_exons ? " outside the mask" : "");
  w.Sp = (S + kPcaTile - 1) / kPcaTile * kPcaTile;
  const int64_t nt = w.Sp / kPcaTile;
  HIP_TRY(w.part.alloc((size_t)kPcaGramSlices * w.Sp * w.Sp * 8));
  HIP_TRY(w.G.alloc((size_t)S * S * 8));
  hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)kPcaGramSlices), dim3(256), 0, st, d_counts, w.sel.as<int32_t>(), w.n, S,
                     w.div.as<double>(), w.centre.as<double>(), w.Sp, w.part.as<double>());
  hipLaunchKernelGGL(k_pca_gram_sum, dim3((unsigned)((S + 255) / 256), (unsigned)S), dim3(256), 0, st, w.part.as<double>(), w.Sp, S, w.G.as<double>());
  HIP_TRY(hipGetLastError());
  if (ev) HIP_TRY(hipEventRecord(ev[2], st));
  return ED_OK;
}

ED_EXPORT int ed_pca_gram(const int32_t* d_counts, int64_t n_exons, int64_t n_samples, const uint8_t* mask_exons, const double* sample_div, double sd_min,
                          double* G_out, double* centre_out, double* div_out, uint8_t* selected_out, int64_t* n_selected, void* stream)
try {
  const int64_t E = n_exons, S = n_samples;
  if (int rc = pca_check_args("ed_pca_gram", d_counts, E, S, sample_div)) return rc;
  if (!G_out) return ed_fail(ED_ERR_INVALID, "ed_pca_gram: NULL output");
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  PcaStage12 w;
  if (int rc = pca_stage12("ed_pca_gram", d_counts, E, S, mask_exons, sample_div, sd_min, st, w, nullptr)) return rc;
  HIP_TRY(hipMemcpyAsync(G_out, w.G.get(), (size_t)S * S * 8, hipMemcpyDeviceToHost, st));
  if (centre_out) HIP_TRY(hipMemcpyAsync(centre_out, w.centre.get(), (size_t)E * 8, hipMemcpyDeviceToHost, st));
  if (div_out) HIP_TRY(hipMemcpyAsync(div_out, w.div.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
  if (selected_out) HIP_TRY(hipMemcpyAsync(selected_out, w.flag.get(), (size_t)E, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_selected) *n_selected = w.n;
  return ED_OK;
}
ED_CATCH("ed_pca_gram")

ED_EXPORT int ed_correct_counts_pca(const int32_t* d_counts, int64_t n_exons, int64_t n_samples, int32_t n_pcs, const uint8_t* mask_exons,
                                    const double* sample_div, const double* exon_mul, const double* sample_mul, double sd_min, double tol,
                                    int32_t max_iter, int32_t* d_out, void* stream)
try {
  const char* who = "ed_correct_counts_pca";
  const int64_t E = n_exons, S = n_samples;
  if (int rc = pca_check_args(who, d_counts, E, S, sample_div)) return rc;
  if (!d_out) return ed_fail(ED_ERR_INVALID, "%s: NULL output", who);
  if (n_pcs < 1) return ed_fail(ED_ERR_INVALID, "%s: nPCs = %d, at least 1", who, (int)n_pcs);
  if (n_pcs > kPcaMaxPcs) return ed_fail(ED_ERR_INVALID, "%s: nPCs = %d, at most %d", who, (int)n_pcs, kPcaMaxPcs);
  if (n_pcs >= S) return ed_fail(ED_ERR_INVALID, "%s: nPCs = %d must be below the number of samples (%lld)", who, (int)n_pcs, (long long)S);
  if (!(tol > 0.0) || max_iter < 1) return ed_fail(ED_ERR_INVALID, "%s: tol = %g, max_iter = %d", who, tol, (int)max_iter);
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  Event pe[5];
  for (auto& e : pe) HIP_TRY(e.create());
  PcaStage12 w;
  if (int rc = pca_stage12(who, d_counts, E, S, mask_exons, sample_div, sd_min, st, w, pe)) return rc;
  const int k = n_pcs;
  if (k >= w.n)
    return ed_fail(ED_ERR_INVALID, "%s: nPCs = %d must be below the number of selected exons (%lld)", who, k, (long long)w.n);
  const int b = (int)std::min<int64_t>(S, std::max(2 * k, k + 8));
  // ---- stage 3 ----
  DevBuf<void> Q, Z, X, Y, T, H, W, Wt, theta, res2, bad;
  const size_t sb = (size_t)S * b * 8, bb = (size_t)b * b * 8;
  HIP_TRY(Q.alloc(sb)); HIP_TRY(Z.alloc(sb)); HIP_TRY(X.alloc(sb)); HIP_TRY(Y.alloc(sb)); HIP_TRY(T.alloc(sb));
  HIP_TRY(H.alloc(bb)); HIP_TRY(W.alloc(bb)); HIP_TRY(Wt.alloc(bb)); HIP_TRY(theta.alloc((size_t)b * 8)); HIP_TRY(res2.alloc((size_t)b * 8));
  HIP_TRY(bad.alloc(4));
  HIP_TRY(hipMemsetAsync(bad.get(), 0, 4, st));
  const int two_in_lds = 2 * bb <= (size_t)128 * 1024;      // b <= 90: the rotations / the inverse next to the matrix in LDS
  const size_t small_lds = two_in_lds ? 2 * bb : bb;
  if (small_lds > 48 * 1024) {
    HIP_TRY(hipFuncSetAttribute((const void*)k_pca_jacobi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds));
    HIP_TRY(hipFuncSetAttribute((const void*)k_pca_chol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds));
  }
  const unsigned sb_blocks = (unsigned)(((int64_t)S * b + 255) / 256);
  // Q <- orthonormal basis of the columns of A (Cholesky QR, twice): A -> T -> Q
  auto orthonormalise = [&](DevBuf<void>& A) -> int {
    double* src = A.as<double>();
    for (int pass = 0; pass < 2; ++pass) {
      double* dst = pass == 0 ? T.as<double>() : Q.as<double>();
      hipLaunchKernelGGL(k_pca_dots, dim3((unsigned)b, (unsigned)b), dim3(256), 0, st, src, (int64_t)1, (int64_t)b, src, (int64_t)b, (int64_t)1, S,
                         H.as<double>(), (int64_t)b);
      hipLaunchKernelGGL(k_pca_chol, dim3(1), dim3(128), small_lds, st, H.as<double>(), b, two_in_lds, W.as<double>(), bad.as<int>());
      hipLaunchKernelGGL(k_pca_rmul, dim3(sb_blocks), dim3(256), 0, st, src, W.as<double>(), S, b, dst);
      src = dst;
    }
    HIP_TRY(hipGetLastError());
    return ED_OK;
  };
  hipLaunchKernelGGL(k_pca_init, dim3(sb_blocks), dim3(256), 0, st, (int64_t)S * b, Y.as<double>());
  if (int rc = orthonormalise(Y)) return rc;
  std::vector<double> h_theta((size_t)b), h_res2((size_t)b);
  int iters = 0, h_bad = 0;
  double rel = std::numeric_limits<double>::infinity();
  bool converged = false;
  while (iters < max_iter) {
    ++iters;
    // Z = G Q; H = Q^T Z; H = W diag(theta) W^T; X = Q W, Y = Z W = G X, residuals
    hipLaunchKernelGGL(k_pca_dots, dim3((unsigned)b, (unsigned)S), dim3(256), 0, st, w.G.as<double>(), S, (int64_t)1, Q.as<double>(), (int64_t)b, (int64_t)1, S,
                       Z.as<double>(), (int64_t)b);
    hipLaunchKernelGGL(k_pca_dots, dim3((unsigned)b, (unsigned)b), dim3(256), 0, st, Q.as<double>(), (int64_t)1, (int64_t)b, Z.as<double>(), (int64_t)b,
                       (int64_t)1, S, H.as<double>(), (int64_t)b);
    hipLaunchKernelGGL(k_pca_jacobi, dim3(1), dim3(128), small_lds, st, H.as<double>(), b, two_in_lds, Wt.as<double>(), W.as<double>(), theta.as<double>());
    hipLaunchKernelGGL(k_pca_rotate, dim3(sb_blocks), dim3(256), 0, st, Q.as<double>(), Z.as<double>(), W.as<double>(), theta.as<double>(), S, b,
                       X.as<double>(), Y.as<double>(), T.as<double>());
    hipLaunchKernelGGL(k_pca_colnorm2, dim3((unsigned)b), dim3(256), 0, st, T.as<double>(), S, b, res2.as<double>());
    HIP_TRY(hipGetLastError());
    // one host round trip per iteration: b + b doubles and a flag (its cost is part of the "eigenvectors" stage time)
    HIP_TRY(hipMemcpyAsync(h_theta.data(), theta.get(), (size_t)b * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_res2.data(), res2.get(), (size_t)b * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_bad, bad.get(), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_bad) return ed_fail(ED_ERR_STATE, "%s: the iteration's basis lost rank after %d iterations (Cholesky pivot not positive)", who, iters);
    if (!(h_theta[0] > 0.0)) return ed_fail(ED_ERR_STATE, "%s: the Gram matrix has no positive eigenvalue (theta_1 = %g)", who, h_theta[0]);
    double worst = 0.0;
    for (int i = 0; i < k; ++i) worst = std::max(worst, h_res2[(size_t)i]);
    rel = std::sqrt(worst) / h_theta[0];
    if (!std::isfinite(rel)) return ed_fail(ED_ERR_STATE, "%s: non-finite residual after %d iterations", who, iters);
    if (rel <= tol) { converged = true; break; }
    if (iters < max_iter) if (int rc = orthonormalise(Y)) return rc;
  }
  const double gap = (k < b && h_theta[(size_t)k] > 0.0) ? h_theta[(size_t)k - 1] / h_theta[(size_t)k] : std::numeric_limits<double>::infinity();
  HIP_TRY(hipEventRecord(pe[3], st));
  // what ed_pca_last_info reports; after a call that did not converge: the stages that ran, [7] the time spent iterating, [8] and [9] zero
  auto save_info = [&](int last_ev) -> int {
    std::lock_guard<std::mutex> lk(g_pca_mu);
    for (auto& v : g_pca_info) v = 0.0;
    g_pca_info[0] = iters; g_pca_info[1] = rel; g_pca_info[2] = (double)w.n; g_pca_info[3] = b; g_pca_info[4] = k;
    float ms = 0.f;
    for (int q = 0; q < last_ev; ++q) { HIP_TRY(hipEventElapsedTime(&ms, pe[q], pe[q + 1])); g_pca_info[5 + q] = ms; }
    if (last_ev == 4) { HIP_TRY(hipEventElapsedTime(&ms, pe[0], pe[4])); g_pca_info[9] = ms; }
    g_pca_info[10] = kPcaGramSlices;
    g_pca_info[11] = (double)(((w.n + kPcaChunk - 1) / kPcaChunk + kPcaGramSlices - 1) / kPcaGramSlices * kPcaChunk);
    g_pca_info[12] = gap;
    g_pca_info[13] = converged ? 1.0 : 0.0;
    for (int i = 0; i <= k && i < b; ++i) g_pca_info[ED_PCA_INFO_THETA + i] = h_theta[(size_t)i];
    g_pca_basis.clear(); g_pca_basis_S = 0; g_pca_basis_k = 0;
    return ED_OK;
  };
  if (!converged) {
    HIP_TRY(hipEventSynchronize(pe[3]));
    if (int rc = save_info(3)) return rc;
    return ed_fail(ED_ERR_STATE, "%s: the subspace iteration did not converge: %d iterations, residual %.3e of theta_1 (tol %.3e), theta_k / theta_k+1 = %.6g",
                   who, iters, rel, tol, gap);
  }
  // ---- stage 4 ----
  DevBuf<void> emul, smul;
  if (exon_mul) {
    HIP_TRY(emul.alloc((size_t)E * 8));
    HIP_TRY(hipMemcpyAsync(emul.get(), exon_mul, (size_t)E * 8, hipMemcpyHostToDevice, st));
  }
  if (sample_mul) {
    HIP_TRY(smul.alloc((size_t)S * 8));
    HIP_TRY(hipMemcpyAsync(smul.get(), sample_mul, (size_t)S * 8, hipMemcpyHostToDevice, st));
  }
  {
    const size_t ulds = (size_t)S * k * 8;
    const int u_in_lds = ulds <= 64 * 1024;
    const unsigned blocks = (unsigned)std::min<int64_t>((E + 3) / 4, 256 * 8);
    hipLaunchKernelGGL(k_pca_residual, dim3(blocks), dim3(256), u_in_lds ? ulds : 0, st, d_counts, E, S, w.div.as<double>(), w.centre.as<double>(),
                       exon_mul ? emul.as<double>() : w.rs.as<double>(), sample_mul ? smul.as<double>() : (const double*)nullptr, X.as<double>(), b, k,
                       u_in_lds, d_out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(pe[4], st));
  std::vector<double> hX((size_t)S * b);
  HIP_TRY(hipMemcpyAsync(hX.data(), X.get(), sb, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (int rc = save_info(4)) return rc;
  {
    std::lock_guard<std::mutex> lk(g_pca_mu);
    g_pca_basis.assign((size_t)S * k, 0.0);
    for (int64_t s = 0; s < S; ++s) for (int j = 0; j < k; ++j) g_pca_basis[(size_t)(s * k + j)] = hX[(size_t)(s * b + j)];
    g_pca_basis_S = S; g_pca_basis_k = k;
  }
  return ED_OK;
}
ED_CATCH("ed_correct_counts_pca")

ED_EXPORT int ed_pca_last_info(double out[ED_PCA_INFO_N])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(g_pca_mu);
  for (int q = 0; q < ED_PCA_INFO_N; ++q) out[q] = g_pca_info[q];
  return ED_OK;
}
ED_CATCH("ed_pca_last_info")

ED_EXPORT int ed_pca_last_basis(double* U_out, int64_t cap, int64_t* n_samples, int32_t* n_pcs)
try {
  std::lock_guard<std::mutex> lk(g_pca_mu);
  if (n_samples) *n_samples = g_pca_basis_S;
  if (n_pcs) *n_pcs = (int32_t)g_pca_basis_k;
  if (U_out) {
    if (cap < (int64_t)g_pca_basis.size()) return ed_fail(ED_ERR_INVALID, "ed_pca_last_basis: room for %lld values, %lld needed", (long long)cap, (long long)g_pca_basis.size());
    for (size_t i = 0; i < g_pca_basis.size(); ++i) U_out[i] = g_pca_basis[i];
  }
  return ED_OK;
}
ED_CATCH("ed_pca_last_basis")
