// edannot.inc -- interval join of a call table against an annotation track: AnnotateExtra (R/annotate_extra.R:41-73) and the cohort's
// self-join, on the device (included at the end of edcore.hip).
//
// A query [qs, qe] on chromosome c and a subject [ss, se] on chromosome c' are a hit iff
//   c == c'                                               chromosomes are ids here (names are matched on the host)
//   qs <= se && ss <= qe                                  findOverlaps(type = "any") on closed integer ranges (:46)
//   (double)ov > min_overlap * (double)(qe - qs)          ov = min(se, qe) - max(qs, ss), no + 1 (:63-65)
//   group filter (optional): the query's group differs from the subject's;  kind filter (optional): the kinds are equal.
//
// The track (ed_annot) is built once: subjects stably sorted by start within their chromosome, pmax[i] = the running maximum of `end` over
// that order (monotone within a chromosome).  For a query, with [co, ce) its chromosome's range of the sorted order,
//   hi = upper bound of qe in start[co, ce)   every subject at hi or beyond starts after qe: ss <= qe fails
//   lo = lower bound of qs in pmax[co, ce)    every subject before lo has end <= pmax < qs: qs <= se fails
// so every hit lies in the window [lo, hi) and nothing outside it is read.  Inside the window ss <= qe holds; qs <= se is tested (a long early
// subject lifts pmax over short later ones).  Sorted position order IS the documented hit order (subject start, caller's index): the sort is stable.
//
// Passes: k_annot_count (a lane per query: the two searches, the window, and -- for windows of at most kAnnotWide subjects -- the count; wider
// windows are put on a list) -> k_annot_count_wide (a wave per listed query, 64 candidates a pass, ballot + popcount) -> exclusive scan of the
// int64 counts (k_annot_scan_block / _sums / _add) -> k_annot_fill / k_annot_fill_wide (the same walks, survivors written at offsets[q] in
// window order; in the wave form a survivor's slot is the popcount of the ballot below its lane, which keeps the order).
// Which form served a query changes nothing in what is written.

namespace {

#ifndef ED_ANNOT_WIDE
#define ED_ANNOT_WIDE 32
#endif
constexpr int kAnnotWide = ED_ANNOT_WIDE;   // windows of more subjects than this go to the wave-per-query kernels (DESIGN 4.15)
constexpr int kAnnotBlock = 256;            // threads of every annot kernel: 256 queries (lane form) or 4 queries (wave form) a workgroup
constexpr int kAnnotScanItems = 4;          // values a thread of k_annot_scan_block owns
constexpr int kAnnotScanBlock = kAnnotBlock * kAnnotScanItems;   // values a workgroup of the scan owns
constexpr int kAnnotWideGrid = 4096;        // most workgroups of a wave-form launch (each wave strides over the list)

struct AnnotTrack {          // device arrays of the sorted track
  const int32_t* start;      // [n] ascending within a chromosome
  const int32_t* end;        // [n]
  const int32_t* pmax;       // [n] running maximum of end within the chromosome
  const int32_t* index;      // [n] position in the caller's order
  const int32_t* group;      // [n] or NULL
  const int32_t* kind;       // [n] or NULL
  const int64_t* chrom_off;  // [n_chrom + 1]
  int32_t n_chrom;
};

struct AnnotQuery {          // device arrays of one query set
  const int32_t* chrom;
  const int32_t* start;
  const int32_t* end;
  const int32_t* group;      // NULL = no group filter
  const int32_t* kind;       // NULL = no kind filter
  int64_t n;
};

// subject p of the window against the query: ss <= qe is implied by p < hi and tested all the same (one compare)
__device__ __forceinline__ bool annot_hit(const AnnotTrack& t, int64_t p, int32_t qs, int32_t qe, double bar, bool fg, int32_t qg, bool fk, int32_t qk)
{
  const int32_t ss = t.start[p], se = t.end[p];
  if (!(qs <= se && ss <= qe)) return false;
  const int64_t ov = (int64_t)(se < qe ? se : qe) - (int64_t)(qs > ss ? qs : ss);
  if (!((double)ov > bar)) return false;
  if (fg && t.group[p] == qg) return false;
  if (fk && t.kind[p] != qk) return false;
  return true;
}

// the window of query q; an unknown chromosome gives the empty window
__device__ __forceinline__ void annot_window(const AnnotTrack& t, int32_t c, int32_t qs, int32_t qe, int64_t& lo_out, int64_t& hi_out)
{
  lo_out = hi_out = 0;
  if (c < 0 || c >= t.n_chrom) return;
  const int64_t co = t.chrom_off[c], ce = t.chrom_off[c + 1];
  int64_t a = co, b = ce;                       // first position in [co, ce) with start > qe
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (t.start[m] <= qe) a = m + 1; else b = m;
  }
  const int64_t hi = a;
  a = co; b = hi;                               // first position in [co, hi) with pmax >= qs (beyond hi nothing is wanted)
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (t.pmax[m] < qs) a = m + 1; else b = m;
  }
  lo_out = a; hi_out = hi;
}

// A lane per query: window, and the count of a narrow one.  Wide queries are appended to wide_list (order irrelevant: every result is written
// at a place that depends on q alone); one atomic per wave.
__global__ void __launch_bounds__(kAnnotBlock)
k_annot_count(AnnotTrack t, AnnotQuery Q, double min_overlap, int32_t* __restrict__ win_lo, int32_t* __restrict__ win_n,
              int64_t* __restrict__ counts, int32_t* __restrict__ wide_list, unsigned int* __restrict__ n_wide)
{
  const int64_t q = (int64_t)blockIdx.x * kAnnotBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool wide = false;
  if (q < Q.n) {
    const int32_t qs = Q.start[q], qe = Q.end[q];
    int64_t lo, hi;
    annot_window(t, Q.chrom[q], qs, qe, lo, hi);
    win_lo[q] = (int32_t)lo;
    win_n[q] = (int32_t)(hi - lo);
    if (hi - lo > kAnnotWide) wide = true;
    else {
      const double bar = min_overlap * (double)((int64_t)qe - (int64_t)qs);
      const bool fg = Q.group != nullptr, fk = Q.kind != nullptr;
      const int32_t qg = fg ? Q.group[q] : 0, qk = fk ? Q.kind[q] : 0;
      int64_t c = 0;
      for (int64_t p = lo; p < hi; ++p) c += annot_hit(t, p, qs, qe, bar, fg, qg, fk, qk) ? 1 : 0;
      counts[q] = c;
    }
  }
  const unsigned long long m = __ballot(wide);
  if (m) {
    unsigned int base = 0;
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) base = atomicAdd(n_wide, (unsigned int)__popcll(m));
    base = __shfl(base, leader, 64);
    if (wide) wide_list[base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = (int32_t)q;
  }
}

// A wave per listed query, 64 candidates a pass.
__global__ void __launch_bounds__(kAnnotBlock)
k_annot_count_wide(AnnotTrack t, AnnotQuery Q, double min_overlap, const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_n,
                   const int32_t* __restrict__ wide_list, const unsigned int* __restrict__ n_wide, int64_t* __restrict__ counts)
{
  const int lane = threadIdx.x & 63;
  const int64_t n_list = (int64_t)*n_wide, step = (int64_t)gridDim.x * (kAnnotBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kAnnotBlock / 64) + (threadIdx.x >> 6); i < n_list; i += step) {
    const int64_t q = wide_list[i];
    const int32_t qs = Q.start[q], qe = Q.end[q];
    const int64_t lo = win_lo[q], hi = lo + win_n[q];
    const double bar = min_overlap * (double)((int64_t)qe - (int64_t)qs);
    const bool fg = Q.group != nullptr, fk = Q.kind != nullptr;
    const int32_t qg = fg ? Q.group[q] : 0, qk = fk ? Q.kind[q] : 0;
    int64_t c = 0;
    for (int64_t base = lo; base < hi; base += 64) {
      const int64_t p = base + lane;
      const bool h = p < hi && annot_hit(t, p, qs, qe, bar, fg, qg, fk, qk);
      c += __popcll(__ballot(h));
    }
    if (lane == 0) counts[q] = c;
  }
}

// Exclusive scan of counts[n] into offsets[n + 1], three launches.  (1) every workgroup scans its kAnnotScanBlock values (a thread owns
// kAnnotScanItems consecutive ones) and leaves its total in bsum; (2) one workgroup turns bsum into its own exclusive scan (a thread owns a
// contiguous range, as k_pca_compact does) and writes the grand total to offsets[n]; (3) every value gets its workgroup's base.
__global__ void __launch_bounds__(kAnnotBlock)
k_annot_scan_block(const int64_t* __restrict__ counts, int64_t n, int64_t* __restrict__ offsets, int64_t* __restrict__ bsum)
{
  __shared__ int64_t sh[kAnnotBlock];
  const int t = threadIdx.x;
  const int64_t i0 = ((int64_t)blockIdx.x * kAnnotBlock + t) * kAnnotScanItems;
  int64_t v[kAnnotScanItems], s = 0;
#pragma unroll
  for (int k = 0; k < kAnnotScanItems; ++k) { v[k] = i0 + k < n ? counts[i0 + k] : 0; s += v[k]; }
  sh[t] = s;
  __syncthreads();
  for (int d = 1; d < kAnnotBlock; d <<= 1) {
    const int64_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  int64_t w = sh[t] - s;
#pragma unroll
  for (int k = 0; k < kAnnotScanItems; ++k) { if (i0 + k < n) offsets[i0 + k] = w; w += v[k]; }
  if (t == kAnnotBlock - 1) bsum[blockIdx.x] = sh[t];
}

__global__ void __launch_bounds__(1024)
k_annot_scan_sums(int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ total_out)
{
  __shared__ int64_t sc[1024];
  const int t = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024, lo = (int64_t)t * per < nb ? (int64_t)t * per : nb, hi = lo + per < nb ? lo + per : nb;
  int64_t c = 0;
  for (int64_t b = lo; b < hi; ++b) c += bsum[b];
  sc[t] = c;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t add = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  int64_t w = sc[t] - c;
  for (int64_t b = lo; b < hi; ++b) { const int64_t x = bsum[b]; bsum[b] = w; w += x; }
  if (t == 1023) *total_out = sc[1023];
}

__global__ void __launch_bounds__(kAnnotBlock)
k_annot_scan_add(int64_t* __restrict__ offsets, int64_t n, const int64_t* __restrict__ bsum)
{
  const int64_t base = bsum[blockIdx.x];
  const int64_t i0 = ((int64_t)blockIdx.x * kAnnotBlock + threadIdx.x) * kAnnotScanItems;
#pragma unroll
  for (int k = 0; k < kAnnotScanItems; ++k) if (i0 + k < n) offsets[i0 + k] += base;
}

// fill, lane form: the narrow queries; survivors in window order
__global__ void __launch_bounds__(kAnnotBlock)
k_annot_fill(AnnotTrack t, AnnotQuery Q, double min_overlap, const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_n,
             const int64_t* __restrict__ offsets, int32_t* __restrict__ hits)
{
  const int64_t q = (int64_t)blockIdx.x * kAnnotBlock + threadIdx.x;
  if (q >= Q.n) return;
  const int64_t lo = win_lo[q], hi = lo + win_n[q];
  if (hi - lo > kAnnotWide) return;
  const int32_t qs = Q.start[q], qe = Q.end[q];
  const double bar = min_overlap * (double)((int64_t)qe - (int64_t)qs);
  const bool fg = Q.group != nullptr, fk = Q.kind != nullptr;
  const int32_t qg = fg ? Q.group[q] : 0, qk = fk ? Q.kind[q] : 0;
  int64_t w = offsets[q];
  const int64_t w_end = offsets[q + 1];       // never written past: the count pass saw the same subjects
  for (int64_t p = lo; p < hi; ++p)
    if (annot_hit(t, p, qs, qe, bar, fg, qg, fk, qk) && w < w_end) hits[w++] = t.index[p];
}

// fill, wave form: a survivor's slot within a pass is the number of surviving lanes below it
__global__ void __launch_bounds__(kAnnotBlock)
k_annot_fill_wide(AnnotTrack t, AnnotQuery Q, double min_overlap, const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_n,
                  const int32_t* __restrict__ wide_list, const unsigned int* __restrict__ n_wide, const int64_t* __restrict__ offsets,
                  int32_t* __restrict__ hits)
{
  const int lane = threadIdx.x & 63;
  const int64_t n_list = (int64_t)*n_wide, step = (int64_t)gridDim.x * (kAnnotBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kAnnotBlock / 64) + (threadIdx.x >> 6); i < n_list; i += step) {
    const int64_t q = wide_list[i];
    const int32_t qs = Q.start[q], qe = Q.end[q];
    const int64_t lo = win_lo[q], hi = lo + win_n[q];
    const double bar = min_overlap * (double)((int64_t)qe - (int64_t)qs);
    const bool fg = Q.group != nullptr, fk = Q.kind != nullptr;
    const int32_t qg = fg ? Q.group[q] : 0, qk = fk ? Q.kind[q] : 0;
    int64_t w = offsets[q];
    const int64_t w_end = offsets[q + 1];
    for (int64_t base = lo; base < hi; base += 64) {
      const int64_t p = base + lane;
      const bool h = p < hi && annot_hit(t, p, qs, qe, bar, fg, qg, fk, qk);
      const unsigned long long m = __ballot(h);
      const int64_t slot = w + __popcll(m & ((1ull << lane) - 1ull));
      if (h && slot < w_end) hits[slot] = t.index[p];
      w += __popcll(m);
    }
  }
}

}  // namespace

struct ed_annot {
  int device = 0;
  int64_t n = 0;
  int32_t n_chrom = 0;
  bool has_group = false, has_kind = false;
  DevBuf<char> d_track;       // ONE allocation: start, end, pmax, index, group, kind (int32 [n] each), then chrom_off (int64 [n_chrom + 1])
  AnnotTrack track{};
  DevBuf<char> d_work;        // ONE grow-only allocation for a query set's arrays (carved in ed_annot_overlaps)
  DevBuf<int32_t> d_hits;     // grow-only
  Stream stream;              // (declared last: it goes first, after ed_annot_destroy has waited for it)
};

ED_EXPORT void ed_annot_destroy(ed_annot* a)
{
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  delete a;
}

ED_EXPORT int64_t ed_annot_n(const ed_annot* a) { return a ? a->n : 0; }

// out = {windows wider than this take the wave form, queries a workgroup of the lane form serves, subjects a wave of the wave form looks at in one
// pass, values a workgroup of the scan owns}: what a test needs to place its shapes on the edges
ED_EXPORT int ed_annot_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_annot_geometry: NULL output");
  out[0] = kAnnotWide; out[1] = kAnnotBlock; out[2] = 64; out[3] = kAnnotScanBlock;
  return ED_OK;
}
ED_CATCH("ed_annot_geometry")

static size_t annot_up(size_t b) { return (b + 255) & ~(size_t)255; }

ED_EXPORT int ed_annot_create(ed_annot** annot, int device, int64_t n, int32_t n_chrom, const int32_t* chrom, const int32_t* start,
                              const int32_t* end, const int32_t* group, const int32_t* kind)
try {
  if (!annot || n < 0 || n_chrom < 0 || (n > 0 && (!chrom || !start || !end)))
    return ed_fail(ED_ERR_INVALID, "ed_annot_create: bad arguments");
  if (n > 2147483647LL) return ed_fail(ED_ERR_INVALID, "ed_annot_create: at most 2^31 - 1 subjects (hits are int32 indices)");
  for (int64_t i = 0; i < n; ++i) {
    if (chrom[i] < 0 || chrom[i] >= n_chrom)
      return ed_fail(ED_ERR_INVALID, "ed_annot_create: subject %lld has chromosome id %d outside 0 .. %d", (long long)i, chrom[i], n_chrom - 1);
    if (start[i] < 0 || end[i] < start[i])
      return ed_fail(ED_ERR_INVALID, "ed_annot_create: subject %lld has start %d, end %d (0 <= start <= end wanted)", (long long)i, start[i], end[i]);
  }
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(device));
  // counting sort by chromosome (stable), then a stable sort by start within each: ties keep the caller's order
  std::vector<int64_t> off((size_t)n_chrom + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++off[(size_t)chrom[i] + 1];
  for (int32_t c = 0; c < n_chrom; ++c) off[(size_t)c + 1] += off[c];
  std::vector<int32_t> idx((size_t)n);
  {
    std::vector<int64_t> at(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; ++i) idx[(size_t)at[chrom[i]]++] = (int32_t)i;
  }
  for (int32_t c = 0; c < n_chrom; ++c)
    std::stable_sort(idx.begin() + off[c], idx.begin() + off[(size_t)c + 1], [start](int32_t a, int32_t b) { return start[a] < start[b]; });
  const int n_arr = 4 + (group ? 1 : 0) + (kind ? 1 : 0);
  const size_t arr = annot_up((size_t)std::max<int64_t>(n, 1) * 4), bytes = arr * n_arr + annot_up(((size_t)n_chrom + 1) * 8);
  std::vector<char> img(bytes, 0);
  int32_t* h_start = (int32_t*)img.data();
  int32_t* h_end = (int32_t*)(img.data() + arr);
  int32_t* h_pmax = (int32_t*)(img.data() + 2 * arr);
  int32_t* h_index = (int32_t*)(img.data() + 3 * arr);
  int32_t* h_group = group ? (int32_t*)(img.data() + 4 * arr) : nullptr;
  int32_t* h_kind = kind ? (int32_t*)(img.data() + (4 + (group ? 1 : 0)) * arr) : nullptr;
  int64_t* h_off = (int64_t*)(img.data() + arr * n_arr);
  for (int32_t c = 0; c < n_chrom; ++c) {
    int32_t run = 0;
    for (int64_t p = off[c]; p < off[(size_t)c + 1]; ++p) {
      const int32_t i = idx[(size_t)p];
      h_start[p] = start[i]; h_end[p] = end[i]; h_index[p] = i;
      run = (p == off[c] || end[i] > run) ? end[i] : run;
      h_pmax[p] = run;
      if (h_group) h_group[p] = group[i];
      if (h_kind) h_kind[p] = kind[i];
    }
  }
  for (int32_t c = 0; c <= n_chrom; ++c) h_off[c] = off[c];
  ed_annot* a = new (std::nothrow) ed_annot;
  if (!a) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  struct Guard { ed_annot* a; ~Guard() { if (a) ed_annot_destroy(a); } } guard{a};   // released on success only (ed_annot_destroy waits for the stream)
  a->device = device; a->n = n; a->n_chrom = n_chrom; a->has_group = group != nullptr; a->has_kind = kind != nullptr;
  if (a->d_track.alloc(bytes) != hipSuccess) {
    return ed_fail(ED_ERR_NOMEM, "ed_annot_create: device allocation of %zu bytes failed", bytes);
  }
  {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    a->stream.reset(st);
  }
  HIP_TRY(hipMemcpyAsync(a->d_track, img.data(), bytes, hipMemcpyHostToDevice, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  char* d = a->d_track;
  a->track.start = (const int32_t*)d;
  a->track.end = (const int32_t*)(d + arr);
  a->track.pmax = (const int32_t*)(d + 2 * arr);
  a->track.index = (const int32_t*)(d + 3 * arr);
  a->track.group = group ? (const int32_t*)(d + 4 * arr) : nullptr;
  a->track.kind = kind ? (const int32_t*)(d + (4 + (group ? 1 : 0)) * arr) : nullptr;
  a->track.chrom_off = (const int64_t*)(d + arr * n_arr);
  a->track.n_chrom = n_chrom;
  guard.a = nullptr;
  *annot = a;
  return ED_OK;
}
ED_CATCH("ed_annot_create")

ED_EXPORT int ed_annot_overlaps(ed_annot* a, int64_t n_q, const int32_t* q_chrom, const int32_t* q_start, const int32_t* q_end,
                                const int32_t* q_group, const int32_t* q_kind, double min_overlap, int64_t* counts, int64_t* offsets,
                                int32_t* hits, int64_t cap, int64_t* n_hits)
try {
  if (!a || n_q < 0 || !n_hits || (n_q > 0 && (!q_chrom || !q_start || !q_end || !counts)) || (hits && cap < 0))
    return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: bad arguments");
  if (n_q > 2147483647LL) return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: at most 2^31 - 1 queries a call");
  if (!(min_overlap >= 0.0) || !std::isfinite(min_overlap))
    return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: min_overlap must be a finite number >= 0 (got %g)", min_overlap);
  if (q_group && !a->has_group) return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: q_group given, but the track was created without groups");
  if (q_kind && !a->has_kind) return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: q_kind given, but the track was created without kinds");
  for (int64_t q = 0; q < n_q; ++q)
    if (q_start[q] < 0 || q_end[q] < q_start[q])
      return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: query %lld has start %d, end %d (0 <= start <= end wanted)", (long long)q, q_start[q], q_end[q]);
  HIP_TRY(hipSetDevice(a->device));
  *n_hits = 0;
  if (n_q == 0) {
    if (offsets) offsets[0] = 0;
    return ED_OK;
  }
  // the query set's device arrays, carved from one block: chrom, start, end, group, kind, win_lo, win_n, wide_list (int32 [n_q] each),
  // counts [n_q], offsets [n_q + 1], bsum [nb] (int64), the wide counter
  const int64_t nb = (n_q + kAnnotScanBlock - 1) / kAnnotScanBlock;
  const size_t a4 = annot_up((size_t)n_q * 4), a8 = annot_up(((size_t)n_q + 1) * 8), ab = annot_up((size_t)nb * 8);
  const size_t need = 8 * a4 + 2 * a8 + ab + 256;
  if (a->d_work.reserve(need) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_annot_overlaps: device allocation of %zu bytes failed", need);
  char* w = a->d_work;
  int32_t* d_qc = (int32_t*)w;
  int32_t* d_qs = (int32_t*)(w + a4);
  int32_t* d_qe = (int32_t*)(w + 2 * a4);
  int32_t* d_qg = (int32_t*)(w + 3 * a4);
  int32_t* d_qk = (int32_t*)(w + 4 * a4);
  int32_t* d_lo = (int32_t*)(w + 5 * a4);
  int32_t* d_wn = (int32_t*)(w + 6 * a4);
  int32_t* d_list = (int32_t*)(w + 7 * a4);
  int64_t* d_counts = (int64_t*)(w + 8 * a4);
  int64_t* d_offsets = (int64_t*)(w + 8 * a4 + a8);
  int64_t* d_bsum = (int64_t*)(w + 8 * a4 + 2 * a8);
  unsigned int* d_nwide = (unsigned int*)(w + 8 * a4 + 2 * a8 + ab);
  hipStream_t st = a->stream;
  const size_t qb = (size_t)n_q * 4;
  HIP_TRY(hipMemcpyAsync(d_qc, q_chrom, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_qs, q_start, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_qe, q_end, qb, hipMemcpyHostToDevice, st));
  if (q_group) HIP_TRY(hipMemcpyAsync(d_qg, q_group, qb, hipMemcpyHostToDevice, st));
  if (q_kind) HIP_TRY(hipMemcpyAsync(d_qk, q_kind, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_nwide, 0, 4, st));
  AnnotQuery Q{d_qc, d_qs, d_qe, q_group ? d_qg : nullptr, q_kind ? d_qk : nullptr, n_q};
  const unsigned int grid_q = (unsigned int)((n_q + kAnnotBlock - 1) / kAnnotBlock);
  const unsigned int grid_w = (unsigned int)std::min<int64_t>((n_q + kAnnotBlock / 64 - 1) / (kAnnotBlock / 64), kAnnotWideGrid);
  hipLaunchKernelGGL(k_annot_count, dim3(grid_q), dim3(kAnnotBlock), 0, st, a->track, Q, min_overlap, d_lo, d_wn, d_counts, d_list, d_nwide);
  hipLaunchKernelGGL(k_annot_count_wide, dim3(grid_w), dim3(kAnnotBlock), 0, st, a->track, Q, min_overlap, d_lo, d_wn, d_list, d_nwide, d_counts);
  hipLaunchKernelGGL(k_annot_scan_block, dim3((unsigned int)nb), dim3(kAnnotBlock), 0, st, d_counts, n_q, d_offsets, d_bsum);
  hipLaunchKernelGGL(k_annot_scan_sums, dim3(1), dim3(1024), 0, st, d_bsum, nb, d_offsets + n_q);
  hipLaunchKernelGGL(k_annot_scan_add, dim3((unsigned int)nb), dim3(kAnnotBlock), 0, st, d_offsets, n_q, d_bsum);
  HIP_TRY(hipGetLastError());
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)n_q * 8, hipMemcpyDeviceToHost, st));
  if (offsets) HIP_TRY(hipMemcpyAsync(offsets, d_offsets, ((size_t)n_q + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&total, d_offsets + n_q, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_hits = total;
  if (!hits) return ED_OK;
  if (total > cap)
    return ed_fail(ED_ERR_INVALID, "ed_annot_overlaps: %lld hits do not fit cap = %lld; hits needs room for %lld entries (nothing was written to it)",
                   (long long)total, (long long)cap, (long long)total);
  if (total == 0) return ED_OK;
  if (a->d_hits.reserve((size_t)total * 4) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_annot_overlaps: device allocation of %zu bytes for the hits failed", (size_t)total * 4);
  hipLaunchKernelGGL(k_annot_fill, dim3(grid_q), dim3(kAnnotBlock), 0, st, a->track, Q, min_overlap, d_lo, d_wn, d_offsets, a->d_hits);
  hipLaunchKernelGGL(k_annot_fill_wide, dim3(grid_w), dim3(kAnnotBlock), 0, st, a->track, Q, min_overlap, d_lo, d_wn, d_list, d_nwide, d_offsets, a->d_hits);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hits, a->d_hits, (size_t)total * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ED_OK;
}
ED_CATCH("ed_annot_overlaps")
