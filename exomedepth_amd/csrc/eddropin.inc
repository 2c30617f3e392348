// eddropin.inc -- the two reference-shaped entries (one sample / one chain per call), built for the call rate an R user of the UNCHANGED
// S4 surface produces: new('ExomeDepth') makes one .Call get_loglike_matrix per sample (R/class_definition.R:184-189), CallCNVs one
// .Call C_hmm per chromosome (R/class_definition.R:354-374 -> R/tools.R:97), i.e. 1 + 24 calls per sample.  Included by edcore.hip.
//
// What a call costs is its fixed overhead, so (round 6):
//   * one process-wide scratch -- a device block, a pinned host block and a stream, grown geometrically, kept between calls (was: six hipMalloc /
//     hipFree pairs and six synchronous hipMemcpy per call); ed_dropin_release() frees it.  Calls are serialised by its mutex (R's API is
//     single-threaded, SURVEY 8b);
//   * the inputs are packed into the pinned block by a few host threads, cross the link as ONE copy and the results come back as one;
//   * C_hmm's forward pass is the quad-lane step of k_viterbi (a lane per target state, src/hmm.cpp:74-88: vit_step_q) on a whole wave instead of
//     one lane reading global memory step by step; the rows it reads -- emissions and log-transitions of a step, 128 bytes -- are made by the
//     host in exactly that shape (the host has to touch every emission anyway to get it into pinned memory, and the log-transitions are host
//     libm calls by contract: they are the reference's own exp() / log() calls, src/hmm.cpp:64, :79) and staged through LDS a tile ahead;
//   * the trace-back (src/hmm.cpp:95-100) is the map composition of k_tb_maps / k_tb_chain / k_tb_paths in one workgroup, the run-length
//     summary (src/hmm.cpp:104-126, quirks kept, see k_hmm_traceback) a per-word summary + one short serial pass.

namespace {

struct DropinScratch {
  std::mutex mu;
  int device = -1;
  DevBuf<char> dev;     // both blocks grow-only
  PinBuf<char> pin;
  Stream st;
  void release()
  {
    if (st) (void)hipStreamSynchronize(st);
    st.reset(); dev.reset(); pin.reset();
    device = -1;
  }
};
// (never destroyed at exit: the HIP runtime may be gone by then; the blocks go with the process)
DropinScratch& dropin_scratch() { static DropinScratch* s = new DropinScratch; return *s; }

// the scratch on the calling thread's current device, at least dev_bytes / pin_bytes large
static int dropin_reserve(DropinScratch& s, size_t dev_bytes, size_t pin_bytes)
{
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  if (s.device != cur) { s.release(); s.device = cur; }
  if (!s.st) {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s.st.reset(st);
  }
  auto grown = [](size_t need, size_t have) { return (std::max(need + need / 2, have * 2) + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1); };
  if (s.dev.bytes() < dev_bytes) {      // (a block in use by the stream's queued work is waited for before it goes)
    if (s.dev) HIP_TRY(hipStreamSynchronize(s.st));
    HIP_TRY(s.dev.reserve(grown(dev_bytes, s.dev.bytes())));
  }
  if (s.pin.bytes() < pin_bytes) {
    if (s.pin) HIP_TRY(hipStreamSynchronize(s.st));
    HIP_TRY(s.pin.reserve(grown(pin_bytes, s.pin.bytes())));
  }
  return ED_OK;
}

// memcpy by up to four host threads (blocks of a megabyte and more: a lone thread moves ~10 GB/s, the link takes 50)
static void dropin_copy(void* dst, const void* src, size_t bytes)
{
  const int nt = bytes >= ((size_t)1 << 20) ? (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 4u)) : 1;
  if (nt == 1) { std::memcpy(dst, src, bytes); return; }
  ed_thread_pool pool;
  for (int t = 1; t < nt; ++t) {
    const size_t a = bytes * t / nt, z = bytes * (t + 1) / nt;
    pool.start([=] { std::memcpy((char*)dst + a, (const char*)src + a, z - a); });
  }
  std::memcpy(dst, src, bytes / nt);
  pool.join();
}

// ---- C_hmm: forward pass -------------------------------------------------------------------------------------------------------------------
// rows [m][4][4] doubles, m = nobs - 1: row r = step i = r + 1 (src/hmm.cpp:58), quad lane j (= target state j; lane 3 repeats lane 0):
//   { probabilities[j * nobs + i], log(trans[0]), log(trans[1]), log(trans[2]) }   (src/hmm.cpp:74-79, trans[] of target state j at this gap)
// The whole wave runs the ONE chain (every quad the same values; quad 0 stores).  bpq [ceil(m / 16)][4]: lane j's 2-bit back-pointers, 16
// steps per word, as k_viterbi leaves them.
constexpr int kHmmTile = 32;      // steps per LDS tile: 32 rows x 128 B = one 16-byte load per lane x 4

__global__ void __launch_bounds__(kWave)
k_hmm_forward(const double2* __restrict__ rows, int64_t m, uint32_t* __restrict__ bpq)
{
  const int lane = threadIdx.x, j = lane & 3;
  __shared__ double2 lds[2][kHmmTile * 8];
  double v = (j == 0 || j == 3) ? 0.0 : -HUGE_VAL;          // src/hmm.cpp:48-52
  const int64_t ntile = (m + kHmmTile - 1) / kHmmTile;
  // (four scalars, not an array: captured by the lambda below an array stays in scratch memory)
  double2 g0 = rows[lane], g1 = rows[64 + lane], g2 = rows[128 + lane], g3 = rows[192 + lane];      // (the block is padded by two tiles: no bounds in here)
  lds[0][lane] = g0; lds[0][64 + lane] = g1; lds[0][128 + lane] = g2; lds[0][192 + lane] = g3;
  __syncthreads();
  auto tile = [&](auto par, auto full, int64_t t, int nsteps) {
    constexpr int P = decltype(par)::value;
    constexpr bool kFull = decltype(full)::value;
    const double2* __restrict__ nx = rows + (t + 1) * (kHmmTile * 8);
    g0 = nx[lane]; g1 = nx[64 + lane]; g2 = nx[128 + lane]; g3 = nx[192 + lane];
    uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
    for (int k = 0; k < kHmmTile; ++k) {
      if (kFull || k < nsteps) {
        const double2 a = lds[P][k * 8 + 2 * j], b = lds[P][k * 8 + 2 * j + 1];
        unsigned fw = vit_step_q(v, a.x, a.y, b.x, b.y);
        asm("" : "+v"(fw));                                                       // (as in k_viterbi: keeps the pointer arithmetic next to its step)
        if (k < 16) w0 |= fw << (2 * (k & 15));
        else w1 |= fw << (2 * (k & 15));
      }
    }
    if (lane < 4) {
      bpq[(t * 2) * 4 + lane] = w0;
      if (kFull || nsteps > 16) bpq[(t * 2 + 1) * 4 + lane] = w1;
    }
    lds[P ^ 1][lane] = g0; lds[P ^ 1][64 + lane] = g1; lds[P ^ 1][128 + lane] = g2; lds[P ^ 1][192 + lane] = g3;
    __syncthreads();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  const int64_t nfull = (m / kHmmTile) & ~(int64_t)1;        // pairs of whole tiles
  int64_t t = 0;
  for (; t < nfull; t += 2) {
    tile(I0{}, std::true_type{}, t, kHmmTile);
    tile(I1{}, std::true_type{}, t + 1, kHmmTile);
  }
  for (; t < ntile; ++t) {
    const int nst = (int)std::min<int64_t>(kHmmTile, m - t * kHmmTile);
    if (t & 1) tile(I1{}, std::false_type{}, t, nst);
    else tile(I0{}, std::false_type{}, t, nst);
  }
}

// ---- C_hmm: trace-back + run-length summary, one workgroup ------------------------------------------------------------------------------------
// Observation i = 1 .. m belongs to word (i - 1) / 16; the last observation is forced to state 0 (src/hmm.cpp:96), tb[i - 1] = from[i][tb[i]].
//   (a) every word: the map {state of its last observation} -> {state of the observation before its first}           (parallel)
//   (b) thread 0: the state of every word's last observation, walking the maps from the end                              (serial, 3 instructions a word)
//   (c) every word: replay its steps -> path (as doubles, src/hmm.cpp:140-142), packed states, and what the word does to the summary's
//       carried values: (last position where a call may start, calls pushed, non-zero states since the last push)        (parallel)
//   (d) thread 0: carried values in front of every word; (e) every word: its calls, in order                              (serial / parallel)
// out block: [0] n_calls (int64), [1 .. 1 + m] path, then the calls as rows {start.p, end.p, type, nexons} (1-based, src/hmm.cpp:150-160)
constexpr int kHmmTbThreads = 256;
constexpr int kHmmTbChunk = 2048;       // words per LDS chunk of the serial passes

__device__ __forceinline__ int hmm_word_steps(int64_t w, int64_t m) { return (int)((m - w * 16 < 16) ? (m - w * 16) : 16); }

__global__ void __launch_bounds__(kHmmTbThreads)
k_hmm_traceback(const uint32_t* __restrict__ bpq, int64_t m, uint8_t* __restrict__ maps, uint8_t* __restrict__ ent, int4* __restrict__ wsum,
                double* __restrict__ out, int64_t cap)
{
  const int tid = threadIdx.x;
  const int64_t nw = (m + 15) / 16;
  int64_t* n_calls_out = reinterpret_cast<int64_t*>(out);
  double* path = out + 1;
  double* calls = out + 1 + (m + 1);
  __shared__ int4 sh[kHmmTbChunk];
  __shared__ int s_first;
  uint8_t* shb = reinterpret_cast<uint8_t*>(sh);
  // (a)
  for (int64_t w = tid; w < nw; w += kHmmTbThreads) {
    const int n = hmm_word_steps(w, m);
    const uint4 bw = reinterpret_cast<const uint4*>(bpq)[w];
    int x0 = 0, x1 = 1, x2 = 2;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
      if (k < n) {
        x0 = (int)((tb_pick(bw, x0) >> (2 * k)) & 3u);
        x1 = (int)((tb_pick(bw, x1) >> (2 * k)) & 3u);
        x2 = (int)((tb_pick(bw, x2) >> (2 * k)) & 3u);
      }
    }
    maps[w] = (uint8_t)(x0 | (x1 << 2) | (x2 << 4));
  }
  __syncthreads();
  // (b)
  int st = 0;
  for (int64_t hi = nw; hi > 0; hi -= kHmmTbChunk) {
    const int64_t lo = hi > kHmmTbChunk ? hi - kHmmTbChunk : 0;
    const int cnt = (int)(hi - lo);
    for (int q = tid; q < cnt; q += kHmmTbThreads) shb[q] = maps[lo + q];
    __syncthreads();
    if (tid == 0) {
      for (int q = cnt - 1; q >= 0; --q) {
        const unsigned mp = shb[q];
        shb[kHmmTbChunk + q] = (uint8_t)st;                   // state of word (lo + q)'s last observation
        st = (int)((mp >> (2 * st)) & 3u);
      }
    }
    __syncthreads();
    for (int q = tid; q < cnt; q += kHmmTbThreads) ent[lo + q] = shb[kHmmTbChunk + q];
    __syncthreads();
  }
  if (tid == 0) { s_first = st; path[0] = (double)st; }       // state of observation 0
  __syncthreads();
  const int first = s_first;
  // (c)
  for (int64_t w = tid; w < nw; w += kHmmTbThreads) {
    const int n = hmm_word_steps(w, m);
    const uint4 bw = reinterpret_cast<const uint4*>(bpq)[w];
    int s = ent[w];
    uint32_t pk = 0;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
      if (k < n) {
        pk |= (uint32_t)s << (2 * k);
        s = (int)((tb_pick(bw, s) >> (2 * k)) & 3u);
      }
    }
    int prev = (w > 0) ? (int)ent[w - 1] : first;
    int last_start = -1, npush = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < n) {
        const int64_t i = w * 16 + 1 + k;
        const int cur = (int)((pk >> (2 * k)) & 3u);
        path[i] = (double)cur;
        const int current = (i == 1) ? 0 : prev;              // src/hmm.cpp:105: `current` starts at 0 whatever tb(0) is
        if (prev != cur) {
          if (current == 0) last_start = (int)i;
          else { ++npush; nz = 0; }
        }
        if (cur != 0) ++nz;
        prev = cur;
      }
    }
    wsum[w] = make_int4(last_start, npush, nz, (int)pk);
  }
  __syncthreads();
  // (d) + (e)
  int c_start = -1, c_nex = 0;
  int64_t c_calls = 0;
  for (int64_t lo = 0; lo < nw; lo += kHmmTbChunk) {
    const int cnt = (int)((nw - lo < kHmmTbChunk) ? (nw - lo) : kHmmTbChunk);
    for (int q = tid; q < cnt; q += kHmmTbThreads) sh[q] = wsum[lo + q];
    __syncthreads();
    if (tid == 0) {
      for (int q = 0; q < cnt; ++q) {
        const int4 u = sh[q];
        sh[q] = make_int4(c_start, c_nex, (int)c_calls, u.w);             // carried values in front of the word (+ its packed states)
        if (u.x >= 0) c_start = u.x;
        c_nex = u.y > 0 ? u.z : c_nex + u.z;
        c_calls += u.y;
      }
    }
    __syncthreads();
    for (int q = tid; q < cnt; q += kHmmTbThreads) {
      const int64_t w = lo + q;
      const int n = hmm_word_steps(w, m);
      const int4 u = sh[q];
      int start = u.x, nex = u.y;
      int64_t kc = u.z;
      const uint32_t pk = (uint32_t)u.w;
      int prev = (w > 0) ? (int)ent[w - 1] : first;
      for (int k = 0; k < n; ++k) {
        const int64_t i = w * 16 + 1 + k;
        const int cur = (int)((pk >> (2 * k)) & 3u);
        const int current = (i == 1) ? 0 : prev;
        if (prev != cur) {
          if (current == 0) start = (int)i;
          else {
            if (kc < cap) {
              double* r = calls + kc * 4;
              r[0] = (double)(start + 1); r[1] = (double)i; r[2] = (double)current; r[3] = (double)nex;     // end = (i - 1) + 1
            }
            ++kc;
            nex = 0;
          }
        }
        if (cur != 0) ++nex;
        prev = cur;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *n_calls_out = c_calls;
}

// The six gap-dependent log-transitions of steps i0 + 1 .. i1 (val [m][6]: target state j -> val[2 j], val[2 j + 1] = log(trans[1]), log(trans[2]) of
// src/hmm.cpp:75-79).  exp() / log() are the host's: the reference's own calls (src/hmm.cpp:64, :79); equal arguments inside a step share one call
// (CallCNVs' matrix, R/class_definition.R:343-347, has three distinct ones per gap).
static void hmm_log_transitions(const double T[9], double L, const int32_t* pos, int64_t i0, int64_t i1, double* val)
{
  for (int64_t r = i0; r < i1; ++r) {
    const int64_t i = r + 1;
    const double dist = double(pos[i]) - double(pos[i - 1]);
    const double d = std::exp(-dist / L);
    double arg[6];
    double* v = val + r * 6;
    for (int jj = 0; jj < 3; ++jj) {
      arg[2 * jj] = d * T[jj * 3 + 1] + (1.0 - d) * T[jj * 3];
      arg[2 * jj + 1] = d * T[jj * 3 + 2] + (1.0 - d) * T[jj * 3];
    }
    for (int q = 0; q < 6; ++q) {
      int same = -1;
      for (int p = 0; p < q; ++p) if (std::memcmp(&arg[p], &arg[q], 8) == 0) { same = p; break; }
      v[q] = same >= 0 ? v[same] : std::log(arg[q]);
    }
  }
}

// rows [i0, i1) of k_hmm_forward's input from the emissions and the log-transitions
static void hmm_pack_rows(const double lt0[3], const double* val, const double* proba, int64_t nobs, int64_t i0, int64_t i1, double* rows)
{
  for (int64_t r = i0; r < i1; ++r) {
    const int64_t i = r + 1;
    const double* v = val + r * 6;
    double* o = rows + r * 16;
    for (int jj = 0; jj < 3; ++jj) {
      o[jj * 4 + 0] = proba[jj * nobs + i];
      o[jj * 4 + 1] = lt0[jj];
      o[jj * 4 + 2] = v[2 * jj];
      o[jj * 4 + 3] = v[2 * jj + 1];
    }
    o[12] = o[0]; o[13] = o[1]; o[14] = o[2]; o[15] = o[3];
  }
}

// CallCNVs calls C_hmm once per chromosome and SAMPLE with the same positions, matrix and length (R/class_definition.R:354-374): the
// log-transitions of a chain -- the host's share of a call, 4 libm calls a step -- are kept for the chains seen last (exact inputs compared, the
// values are the ones the first call computed).  Guarded by the scratch's mutex.
struct HmmLtCache {
  struct Entry {
    uint64_t hash = 0, stamp = 0;
    double T[9], L = 0;
    std::vector<int32_t> pos;
    std::vector<double> val;
  };
  std::vector<Entry> e;
  uint64_t clock = 0;
  size_t bytes = 0;
  static constexpr size_t kMaxEntries = 64, kMaxBytes = (size_t)96 << 20;
  static uint64_t hash_of(const int32_t* pos, int64_t n, const double T[9], double L)
  {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)n;
    auto mix = [&](uint64_t x) { h ^= x; h *= 0xff51afd7ed558ccdull; h ^= h >> 29; };
    int64_t i = 0;
    for (; i + 1 < n; i += 2) { uint64_t x; std::memcpy(&x, pos + i, 8); mix(x); }
    if (i < n) mix((uint64_t)(uint32_t)pos[i]);
    for (int q = 0; q < 9; ++q) { uint64_t x; std::memcpy(&x, &T[q], 8); mix(x); }
    uint64_t x; std::memcpy(&x, &L, 8); mix(x);
    return h;
  }
  const double* find(const int32_t* pos, int64_t n, const double T[9], double L, uint64_t h)
  {
    for (auto& en : e)
      if (en.hash == h && (int64_t)en.pos.size() == n && en.L == L && std::memcmp(en.T, T, 72) == 0 && std::memcmp(en.pos.data(), pos, (size_t)n * 4) == 0) {
        en.stamp = ++clock;
        return en.val.data();
      }
    return nullptr;
  }
  double* insert(const int32_t* pos, int64_t n, const double T[9], double L, uint64_t h)
  {
    const size_t need = (size_t)n * 4 + (size_t)(n - 1) * 48;
    while (!e.empty() && (e.size() >= kMaxEntries || bytes + need > kMaxBytes)) {
      size_t old = 0;
      for (size_t q = 1; q < e.size(); ++q) if (e[q].stamp < e[old].stamp) old = q;
      bytes -= e[old].pos.size() * 4 + e[old].val.size() * 8;
      e.erase(e.begin() + (std::ptrdiff_t)old);
    }
    Entry en;                                  // (complete before it is listed: an allocation failure leaves the cache as it was)
    en.hash = h; en.stamp = ++clock; en.L = L;
    std::memcpy(en.T, T, 72);
    en.pos.assign(pos, pos + n);
    en.val.resize((size_t)(n - 1) * 6);
    e.push_back(std::move(en));
    bytes += need;
    return e.back().val.data();
  }
  void clear() { e.clear(); bytes = 0; }
};
HmmLtCache& hmm_lt_cache() { static HmmLtCache* c = new HmmLtCache; return *c; }

}  // namespace

ED_EXPORT void ed_dropin_release(void)
{
  DropinScratch& s = dropin_scratch();
  std::lock_guard<std::mutex> lock(s.mu);
  s.release();
  hmm_lt_cache().clear();
}

// ---- drop-in 1: get_loglike_matrix ---------------------------------------------------------
ED_EXPORT int ed_get_loglike_matrix(const double* phi, const double* expected, const int32_t* total,
                                    const int32_t* observed, int64_t n, double mixture, double* out,
                                    int64_t* n_gsl_errors)
try {
  if (n < 0 || (n > 0 && (!phi || !expected || !total || !observed || !out)))
    return ed_fail(ED_ERR_INVALID, "ed_get_loglike_matrix: NULL buffer or negative n");
  if (int rc = require_device()) return rc;
  if (n_gsl_errors) *n_gsl_errors = 0;
  if (n == 0) return ED_OK;
  DropinScratch& s = dropin_scratch();
  std::lock_guard<std::mutex> lock(s.mu);
  // The rows go in pieces (four from 65 536 rows on), so that the link carries piece k while the host threads gather piece k + 1 and the results of
  // piece k come back under the kernel of k + 1.  A piece of k rows is one block each way, device and pinned alike:
  //   in  [ phi k | expected k | total k | observed k ]  (24 k bytes)       back  [ k x 3 column-major ] (24 k bytes); the error counter behind the last piece's
  const size_t N = (size_t)n;
  const int64_t piece = n >= ((int64_t)1 << 16) ? ((n + 3) / 4 + 1) & ~(int64_t)1 : n;       // (even: the int32 parts stay 8-byte aligned)
  const int np = (int)((n + piece - 1) / piece);
  if (int rc = dropin_reserve(s, N * 48 + 16, N * 48 + 16)) return rc;
  char *hin = s.pin, *hout = s.pin + N * 24, *din = s.dev, *dout = s.dev + N * 24;
  unsigned long long* dnerr = reinterpret_cast<unsigned long long*>(dout + N * 24);
  HIP_TRY(hipMemsetAsync(dnerr, 0, 8, s.st));
  for (int p = 0; p < np; ++p) {
    const size_t r0 = (size_t)p * (size_t)piece, k = std::min((size_t)piece, N - r0), o = r0 * 24;
    dropin_copy(hin + o, phi + r0, k * 8);
    dropin_copy(hin + o + k * 8, expected + r0, k * 8);
    dropin_copy(hin + o + k * 16, total + r0, k * 4);
    dropin_copy(hin + o + k * 20, observed + r0, k * 4);
    HIP_TRY(hipMemcpyAsync(din + o, hin + o, k * 24, hipMemcpyHostToDevice, s.st));
    hipLaunchKernelGGL(k_emit_rows, dim3((unsigned)((k + kEmitBlock - 1) / kEmitBlock)), dim3(kEmitBlock), 0, s.st,
                       reinterpret_cast<const double*>(din + o), reinterpret_cast<const double*>(din + o + k * 8),
                       reinterpret_cast<const int32_t*>(din + o + k * 16), reinterpret_cast<const int32_t*>(din + o + k * 20), (int64_t)k, mixture,
                       reinterpret_cast<double*>(dout + o), dnerr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hout + o, dout + o, k * 24 + (p == np - 1 ? 8 : 0), hipMemcpyDeviceToHost, s.st));
  }
  // one wait; the scatter into the caller's n x 3 matrix (column-major: three segments per piece)
  HIP_TRY(hipStreamSynchronize(s.st));
  for (int p = 0; p < np; ++p) {
    const size_t r0 = (size_t)p * (size_t)piece, k = std::min((size_t)piece, N - r0), o = r0 * 24;
    for (int st = 0; st < 3; ++st) dropin_copy(out + r0 + N * st, hout + o + (size_t)st * k * 8, k * 8);
  }
  unsigned long long ne = 0;
  std::memcpy(&ne, hout + N * 24, 8);
  if (n_gsl_errors) *n_gsl_errors = (int64_t)ne;
  return ED_OK;
}
ED_CATCH("ed_get_loglike_matrix")

// ---- drop-in 2: C_hmm ----------------------------------------------------------------------
ED_EXPORT int ed_hmm(int32_t nstates, int32_t nobs, const double* transitions, const double* probabilities,
                     const int32_t* positions, double expected_length, double* path_out, double* calls_out,
                     int64_t calls_cap, int64_t* n_calls)
try {
  if (nstates != 3) return ed_fail(ED_ERR_INVALID, "ERROR: The code must assume 3 states");  // src/hmm.cpp:37-40
  if (nobs < 0 || calls_cap < 0 || !n_calls || (nobs > 0 && (!transitions || !probabilities || !positions || !path_out)))
    return ed_fail(ED_ERR_INVALID, "ed_hmm: bad arguments");
  if (calls_cap > 0 && !calls_out) return ed_fail(ED_ERR_INVALID, "ed_hmm: calls_out is NULL");
  if (int rc = require_device()) return rc;
  *n_calls = 0;
  if (nobs == 0) return ED_OK;
  if (nobs == 1) { path_out[0] = 0.0; return ED_OK; }                                         // the forced last state (src/hmm.cpp:96), nothing to call
  const int64_t m = (int64_t)nobs - 1, nw = (m + 15) / 16;
  // a chain cannot hold more calls than it has steps (a call ends wherever a non-zero state is left, 1 -> 2 switches included)
  const int64_t cap = std::min<int64_t>(calls_cap, m);
  DropinScratch& s = dropin_scratch();
  std::lock_guard<std::mutex> lock(s.mu);
  // device: [ rows (m + two tiles of padding: the forward pass prefetches a tile ahead) x 128 B | out: n_calls, path, call rows | bpq nw x 16 B | wsum nw x 16 B | maps nw | ent nw ]
  const size_t rows_bytes = (size_t)(m + 2 * kHmmTile) * 128, out_bytes = (size_t)(1 + (m + 1) + 4 * cap) * 8;
  const size_t o_out = rows_bytes, o_bpq = o_out + ((out_bytes + 15) & ~(size_t)15), o_wsum = o_bpq + (size_t)(nw + 2) * 16, o_maps = o_wsum + (size_t)nw * 16,
               o_ent = o_maps + (((size_t)nw + 15) & ~(size_t)15), dev_bytes = o_ent + (size_t)nw + 16;
  if (int rc = dropin_reserve(s, dev_bytes, rows_bytes + out_bytes)) return rc;
  double* hrows = reinterpret_cast<double*>(s.pin.get());
  double* hout = reinterpret_cast<double*>(s.pin + rows_bytes);
  {
    const double lt0[3] = {std::log(transitions[0]), std::log(transitions[3]), std::log(transitions[6])};     // log(trans[0]) = log T[0, j] (src/hmm.cpp:74, :79)
    HmmLtCache& cache = hmm_lt_cache();
    const uint64_t h = HmmLtCache::hash_of(positions, nobs, transitions, expected_length);
    const double* val = cache.find(positions, nobs, transitions, expected_length, h);
    double* fresh = val ? nullptr : cache.insert(positions, nobs, transitions, expected_length, h);
    // (a thread costs ~20 us to start: two from 8 192 steps on, four from 16 384)
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(), 4, m / 4096}));
    ed_thread_pool pool;
    auto part = [&](int t) noexcept {
      const int64_t i0 = m * t / nt, i1 = m * (t + 1) / nt;
      if (fresh) hmm_log_transitions(transitions, expected_length, positions, i0, i1, fresh);
      hmm_pack_rows(lt0, val ? val : fresh, probabilities, nobs, i0, i1, hrows);
    };
    for (int t = 1; t < nt; ++t) pool.start(part, t);
    part(0);
    pool.join();
  }
  HIP_TRY(hipMemcpyAsync(s.dev, hrows, (size_t)m * 128, hipMemcpyHostToDevice, s.st));
  hipLaunchKernelGGL(k_hmm_forward, dim3(1), dim3(kWave), 0, s.st, reinterpret_cast<const double2*>(s.dev.get()), m, reinterpret_cast<uint32_t*>(s.dev + o_bpq));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_hmm_traceback, dim3(1), dim3(kHmmTbThreads), 0, s.st, reinterpret_cast<const uint32_t*>(s.dev + o_bpq), m,
                     reinterpret_cast<uint8_t*>(s.dev + o_maps), reinterpret_cast<uint8_t*>(s.dev + o_ent), reinterpret_cast<int4*>(s.dev + o_wsum),
                     reinterpret_cast<double*>(s.dev + o_out), cap);
  HIP_TRY(hipGetLastError());
  // the count, the path and the first call rows in one copy; a second one only for a chain with more calls than that
  const int64_t first_rows = std::min<int64_t>(cap, 256);
  HIP_TRY(hipMemcpyAsync(hout, s.dev + o_out, (size_t)(1 + (m + 1) + 4 * first_rows) * 8, hipMemcpyDeviceToHost, s.st));
  HIP_TRY(hipStreamSynchronize(s.st));
  int64_t k = 0;
  std::memcpy(&k, hout, 8);
  const int64_t kept = std::min(k, cap);
  if (kept > first_rows) {
    HIP_TRY(hipMemcpyAsync(hout + 1 + (m + 1) + 4 * first_rows, s.dev + o_out + (size_t)(1 + (m + 1) + 4 * first_rows) * 8, (size_t)(kept - first_rows) * 32,
                           hipMemcpyDeviceToHost, s.st));
    HIP_TRY(hipStreamSynchronize(s.st));
  }
  std::memcpy(path_out, hout + 1, (size_t)nobs * 8);
  const double* rows = hout + 1 + (m + 1);
  for (int64_t i = 0; i < std::min(kept, calls_cap); ++i)
    for (int c = 0; c < 4; ++c) calls_out[(size_t)c * calls_cap + i] = rows[i * 4 + c];      // column-major cap x 4 (src/hmm.cpp:135, :150-160)
  *n_calls = k;
  return ED_OK;
}
ED_CATCH("ed_hmm")
