// The mixture profile: the log-evidence of every (pair, chromosome) chain at up to 16 values of the pair's tumour fraction, straight from
// the counts -- no likelihood matrix is written (DESIGN.md 4.21).
//
// The model and its log-evidence are edpost.inc's (header comment): HMM states 0 normal, 1 deletion, 2 duplication, alpha_0 = (0, -inf, -inf),
//   alpha_i(j) = e_i(j) + LSE_k(alpha_{i-1}(k) + lt_i[k->j])    i = 1 .. m          logZ = LSE_k(alpha_m(k) + lt_{m+1}[k->0])
// with lse3's conventions for NaN and all -inf.  The emissions are the strict mode's, bit for bit (k_emit_rows / k_emit_verify):
//   e_i(state) = lnbeta(a1 + obs_i, (a2 + tot_i) - obs_i) - lnbeta(a1, a2),   (a1, a2) = shape_params(state_props(expected, mixture)[state], sd)
// The normal state's expected proportion does not depend on the mixture: one column serves every grid point.  lnbeta(a1, a2) does not
// depend on the exon: once per (pair, grid point, state).
//
// Geometry (ed_mix_plan.hpp): a workgroup of four waves per (pair, chromosome).  Wave 0 walks the chain, a quad of lanes per grid point
// as k_fb_forward's quads walk samples (lane j owns state j, lane 3 shadows state 0; quads beyond the grid shadow its last point and
// store nothing).  Waves 1 .. 3 evaluate the next tile of 64 exons x (1 + 2 G) emissions into LDS meanwhile -- a column a wave and
// pass, an exon a lane, so (a1, a2) and the branches of lnbeta are mostly wave-uniform -- and park the tile's log-transitions next
// to it: the chain wave reads nothing but LDS.  Two tiles, one barrier a tile.  A lane beyond the chain's last exon loads and evaluates
// nothing: no load leaves the chain.
// One operation order per (pair, chromosome, grid point), no atomics, nothing shared between chains: the bits of a value depend on
// (counts, phi, expected, mixture) of its pair alone -- not on S, G, the grid point's index, the other pairs or the count layout.

namespace {

__global__ void __launch_bounds__(edmix::kThreads)
k_mix_profile(const int32_t* __restrict__ test, const int32_t* __restrict__ ref, int64_t ce, int64_t cs,   // count (e, s) at e * ce + s * cs
              const double* __restrict__ phi, const double* __restrict__ expected, const double* __restrict__ grid, int G,
              const double* __restrict__ lt4, double c0, double c1, const int32_t* __restrict__ chrom_off,
              const int32_t* __restrict__ job_chrom, int32_t C, int64_t S, double* __restrict__ logev)
{
  using namespace edmix;
  __shared__ double s_em[2][kTile * kRowStride];    // [exon][column]
  __shared__ double s_lt[2][kTile * kLtStride];     // [exon](A, B, C, -)
  __shared__ double s_cc[3][kRowStride];            // per column a1, a2, lnbeta(a1, a2)
  __shared__ double logt[ED_PM_LOGT_N * 3];
  static_assert(sizeof(double) * ED_PM_LOGT_N * 3 == kLogTableBytes, "ed_mix_plan.hpp: kLogTableBytes");
  static_assert(lds_bytes() <= kLdsLimit, "the tiles do not fit static shared memory");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s = blockIdx.x;
  const int c = job_chrom[blockIdx.y];
  const int64_t lo = chrom_off[c];
  const int m = chrom_off[c + 1] - chrom_off[c];    // > 0: an empty chromosome is in no job
  const int ncol = n_cols(G);
  {
    const double T[ED_PM_LOGT_N][3] = ED_PM_LOGT_ROWS;
    for (int i = tid; i < ED_PM_LOGT_N * 3; i += kThreads) logt[i] = (&T[0][0])[i];
  }
  if (tid < ncol) {                                 // column tid: normal, or (deletion, duplication) at grid point (tid - 1) / 2
    const double ex = expected[s];
    const double sd = __builtin_sqrt((phi[s] * ex) * (1. - ex));
    const int g = tid ? (tid - 1) >> 1 : 0;
    double ep[3];
    state_props(ex, grid[(int64_t)g * S + s], ep);
    const double e1 = tid ? (((tid - 1) & 1) ? ep[2] : ep[0]) : ep[1];
    double a1, a2;
    shape_params(e1, sd, a1, a2);
    int f = 0;
    s_cc[0][tid] = a1;
    s_cc[1][tid] = a2;
    s_cc[2][tid] = edsf::lnbeta(a1, a2, &f);
  }
  __syncthreads();

  // waves 1 .. 3: tile t into buffer `buf`; lane = exon of the tile
  auto fill = [&](int t, int buf) {
    const int cnt = tile_count(m, t);
    if (lane >= cnt) return;
    const int i = tile_first(t) + lane;             // exon of the chain, < m
    const int ew = wave - 1;
    const int64_t at = (lo + i) * ce + s * cs;
    const int32_t obs = test[at];
    const int32_t tot = obs + ref[at];
    if (ew == 0) {                                  // the gap of exon i: lo + c + i; its row is (A, A), (B, C), (C, B), (A, A)
      const double* __restrict__ r = lt4 + (lo + c + i) * 8;
      s_lt[buf][lane * kLtStride + 0] = r[0];
      s_lt[buf][lane * kLtStride + 1] = r[2];
      s_lt[buf][lane * kLtStride + 2] = r[3];
    }
#pragma unroll 1
    for (int col = ew; col < ncol; col += kEmitWaves) {
      const double a1 = s_cc[0][col], a2 = s_cc[1][col], v0 = s_cc[2][col];
      int f1 = 0;
      const double v1 = edsf::lnbeta(a1 + (double)obs, (a2 + (double)tot) - (double)obs, &f1);
      s_em[buf][lane * kRowStride + col] = v1 - v0;
    }
  };

  // wave 0: the chain
  const int j = lane & 3, q = lane >> 2;
  const int g = quad_grid(q, G);
  const bool st0 = (j == 0 || j == 3);
  const int col = st0 ? 0 : (j == 1 ? col_del(g) : col_dup(g));
  const int ix = (j == 1) ? 1 : ((j == 2) ? 2 : 0);      // into state j from deletion: A, B, C, A
  const int iy = (j == 1) ? 2 : ((j == 2) ? 1 : 0);      // ... from duplication:       A, C, B, A
  const double t0 = st0 ? c0 : c1;
  double al = st0 ? 0.0 : -HUGE_VAL;
  double Aend = 0.0;
  if (wave == 0) Aend = lt4[(lo + c + m) * 8];           // the closing step's A
  auto step = [&](double e, double lx, double ly) {
    const double a0 = quad_bcast<0>(al), a1 = quad_bcast<1>(al), a2 = quad_bcast<2>(al);
    al = e + lse3(a0 + t0, a1 + lx, a2 + ly, logt);
  };

  if (wave != 0) fill(0, 0);
  __syncthreads();
  const int nt = n_tiles(m);
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (wave == 0) {
      const int cnt = tile_count(m, t);
      const double* em = &s_em[buf][col];
      const double* lt = &s_lt[buf][0];
      int k = 0;
      for (; k + 8 <= cnt; k += 8) {                     // eight steps' operands first, so that their LDS reads overlap the steps
        double er[8], lx[8], ly[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          er[u] = em[(k + u) * kRowStride];
          lx[u] = lt[(k + u) * kLtStride + ix];
          ly[u] = lt[(k + u) * kLtStride + iy];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) step(er[u], lx[u], ly[u]);
      }
      for (; k < cnt; ++k) step(em[k * kRowStride], lt[k * kLtStride + ix], lt[k * kLtStride + iy]);
    } else if (t + 1 < nt) {
      fill(t + 1, buf ^ 1);
    }
    __syncthreads();
  }
  if (wave == 0) {
    const double a0 = quad_bcast<0>(al), a1 = quad_bcast<1>(al), a2 = quad_bcast<2>(al);
    const double lz = lse3(a0 + c0, a1 + Aend, a2 + Aend, logt);   // logZ = LSE_k(alpha_m(k) + lt_{m+1}[k->0])
    if (quad_live(q, G) && j == 0) logev[((int64_t)g * C + c) * S + s] = lz;
  }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
// The plan's launch rows, made and uploaded on the first request: once, under the plan's lock.  (A synchronous copy: the table is
// complete on the device when this returns, whatever stream reads it.)
static int ensure_mix_jobs(const ed_plan* p)
{
  std::lock_guard<std::mutex> lock(p->mix_mu);
  if (p->n_mix_jobs >= 0) return ED_OK;
  const std::vector<int32_t> jobs = edmix::job_order(p->C, p->chrom_off.data());
  DevBuf<int32_t> d;
  if (d.alloc(jobs.size() * 4) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "mixture profile: cannot allocate %lld launch rows", (long long)jobs.size());
  if (!jobs.empty()) HIP_TRY(hipMemcpy(d.get(), jobs.data(), jobs.size() * 4, hipMemcpyHostToDevice));
  p->d_mix_jobs = std::move(d);
  p->n_mix_jobs = (int32_t)jobs.size();
  return ED_OK;
}

ED_EXPORT int ed_plan_mixture_profile(const ed_plan* p, const int32_t* d_test, const int32_t* d_ref, int layout, int64_t n_samples,
                                      const double* d_phi, const double* d_expected, const double* d_grid, int n_grid, double* d_logev,
                                      void* stream)
try {
  if (!p) return ed_fail(ED_ERR_INVALID, "ed_plan_mixture_profile: NULL plan");
  if (n_grid < 1 || n_grid > edmix::kMaxGrid)
    return ed_fail(ED_ERR_INVALID, "ed_plan_mixture_profile: n_grid = %d is outside 1 .. %d", n_grid, edmix::kMaxGrid);
  if (int rc = check_counts_args("ed_plan_mixture_profile", layout, n_samples)) return rc;
  if (!d_test || !d_ref || !d_phi || !d_expected || !d_grid || !d_logev) return ed_fail(ED_ERR_INVALID, "ed_plan_mixture_profile: NULL array");
  if (p->C > 65535) return ed_fail(ED_ERR_INVALID, "ed_plan_mixture_profile: more than 65535 chromosomes");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if (p->C <= 0) return ED_OK;
  if (int rc = ensure_mix_jobs(p)) return rc;
  const int64_t S = n_samples;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_logev, 0, (size_t)n_grid * p->C * S * 8, st));       // an empty chromosome is in no job: its log-evidence is 0
  if (p->n_mix_jobs <= 0) return ED_OK;
  const CountStrides cst = count_strides(layout, p->E, S);
  hipLaunchKernelGGL(k_mix_profile, dim3((unsigned)S, (unsigned)p->n_mix_jobs), dim3(edmix::kThreads), 0, st, d_test, d_ref,
                     cst.ce, cst.cs, d_phi, d_expected, d_grid, n_grid, (const double*)p->d_lt3.get(),
                     p->c0, p->c1, (const int32_t*)p->d_chrom_off.get(), (const int32_t*)p->d_mix_jobs.get(), p->C, S, d_logev);
  HIP_TRY(hipGetLastError());
  return ED_OK;
}
ED_CATCH("ed_plan_mixture_profile")

// out = {exons of a tile, grid points a launch takes, pairs a workgroup serves, bytes of LDS of a workgroup}: what a test needs to place
// its shapes on the edges
ED_EXPORT int ed_mix_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_mix_geometry: NULL output");
  out[0] = edmix::kTile; out[1] = edmix::kMaxGrid; out[2] = edmix::kPairsPerWg; out[3] = edmix::lds_bytes();
  return ED_OK;
}
ED_CATCH("ed_mix_geometry")
