// edreadcount.inc -- reads per exon from BAM record fields: getBamCounts (countBamInGRanges.exomeDepth, R/countBamInGranges.R:176-248) and
// count.everted.reads (countBam.everted, :120-142), on the device (included at the end of edcore.hip).  DESIGN 4.17.
//
// A record gives at most one fragment [fs, fe] (closed, 1-based) on its own chromosome; an exon [xs, xe] counts the fragments of its chromosome
// with fs <= xe && fe >= xs (countOverlaps, type "any").  For any set of intervals on one chromosome
//   count(exon) = #{fs <= xe} - #{fe < xs}
// because a fragment that ends before the exon starts also starts before the exon ends (fs <= fe < xs <= xe): the second set lies inside the
// first.  Nothing is assumed about the order of the records, about overlapping exons or about fragment lengths.
//
// The object (ed_readcount) holds, per chromosome, the exon ends sorted ascending and the exon starts sorted ascending, the exon at every position
// of the end order and every exon's position in the start order.  Passes:
//   k_rcnt_bin     a lane per record: the mode's filter, the fragment, refID -> target chromosome, then two binary searches --
//                  rA = first sorted end >= fs, rB = first sorted start > fe -- and histA[rA] += 1, histB[rB] += 1 (uint32, one slot per exon; a
//                  rank equal to the chromosome's exon count is dropped: that fragment is in neither set of any exon).  Equal ranks of
//                  neighbouring lanes -- the rule in a coordinate-sorted file -- are merged in the wavefront: one atomic per run.
//   k_rcnt_finish  a workgroup per chromosome: inclusive scan of both histograms in place, then for the exon at end-order position p
//                  counts[column][exon] += cumA[p] - cumB[start rank of exon]  (#{fs <= xe} = cumA at the exon's end rank, #{fe < xs} = cumB at its
//                  start rank, ties included: rA is a lower bound, rB an upper bound), then the histograms are cleared.
// Integer arithmetic throughout: the counts do not depend on the order of the records, on how they were cut into chunks, or on the run.

namespace {

constexpr int kRcntBlock = 256;                              // threads of k_rcnt_bin
constexpr int kRcntItems = 4;                                // records a thread of k_rcnt_bin takes (a workgroup-wide stride apart)
constexpr int kRcntPerGroup = kRcntBlock * kRcntItems;       // records a workgroup of k_rcnt_bin takes
constexpr int kRcntFinishBlock = 1024;                       // threads of k_rcnt_finish, and values of one step of its scan
constexpr int64_t kRcntChunk = (int64_t)1 << 22;             // records of one staged upload (64 MiB a staging set)

struct RcntTable {             // device arrays of the exon table
  const int32_t* ends;         // [n] ascending within a chromosome
  const int32_t* starts;       // [n] ascending within a chromosome
  const int32_t* end_exon;     // [n] the exon (caller's index) at a position of the end order
  const int32_t* start_rank;   // [n] an exon's position in the start order
  const int32_t* chrom_off;    // [n_chrom + 1]
  int32_t n_chrom;
};

// One add per run of equal slots over neighbouring lanes (slot < 0: nothing to add).  Every lane of the wavefront calls it.
__device__ __forceinline__ void rcnt_merged_add(unsigned int* __restrict__ hist, int32_t slot)
{
  const int lane = threadIdx.x & 63;
  const int32_t prev = __shfl_up(slot, 1, 64);
  const bool head = lane == 0 || prev != slot;
  const unsigned long long heads = __ballot(head);
  if (head && slot >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);   // heads of the runs after this one
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    atomicAdd(&hist[slot], (unsigned int)(next - lane));
  }
}

// mode 0: getBamCounts' rule (R/countBamInGranges.R:218-243); mode 1: the everted rule (:127-136).  flag_mapq = flag | mapq << 16.
__device__ __forceinline__ bool rcnt_fragment(int mode, int32_t pos, int32_t tlen, uint32_t flag_mapq, int32_t min_mapq, int32_t read_width,
                                              int64_t& fs, int64_t& fe)
{
  const uint32_t flag = flag_mapq & 0xffffu;
  const int32_t mapq = (int32_t)((flag_mapq >> 16) & 0xffu);
  const int64_t pos1 = (int64_t)pos + 1;
  if (mapq == 255) return false;                                           // "not available": an NA in R (a stated deviation, INTEGRATION)
  if (mode == 0) {
    if (!(mapq > min_mapq)) return false;
    if (flag & 0x1u) {                                                     // paired: proper pair, both mapped, primary, no duplicate
      if (!(flag & 0x2u) || (flag & (0x4u | 0x8u | 0x100u | 0x400u))) return false;
      if (!(tlen > 0)) return false;
      fs = pos1; fe = pos1 + (int64_t)tlen;                                // one longer than the template, as the reference has it
    } else {
      if (flag & (0x4u | 0x100u | 0x400u)) return false;
      fs = pos1; fe = pos1 + (int64_t)read_width;
    }
    return true;
  }
  if (!(flag & 0x1u) || (flag & (0x2u | 0x4u | 0x100u | 0x400u))) return false;
  if (!(mapq >= min_mapq) || pos < 0) return false;
  if (!(tlen > -100000 && tlen < 100000)) return false;
  const bool reverse = (flag & 0x10u) != 0;
  if (!((!reverse && tlen < 0) || (reverse && tlen > 0))) return false;
  const int64_t other = pos1 + (int64_t)tlen;
  fs = pos1 < other ? pos1 : other;
  fe = pos1 < other ? other : pos1;
  return true;
}

__global__ void __launch_bounds__(kRcntBlock)
k_rcnt_bin(RcntTable t, const int32_t* __restrict__ refid, const int32_t* __restrict__ pos, const int32_t* __restrict__ tlen,
           const uint32_t* __restrict__ flag_mapq, int64_t n, const int32_t* __restrict__ ref_to_chrom, int32_t n_ref, int mode,
           int32_t min_mapq, int32_t read_width, unsigned int* __restrict__ histA, unsigned int* __restrict__ histB)
{
  const int64_t base = (int64_t)blockIdx.x * kRcntPerGroup + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kRcntItems; ++k) {
    const int64_t i = base + (int64_t)k * kRcntBlock;
    int32_t slotA = -1, slotB = -1;
    if (i < n) {
      const int32_t r = refid[i];
      const int32_t c = (r >= 0 && r < n_ref) ? ref_to_chrom[r] : -1;
      int64_t fs = 0, fe = 0;
      if (c >= 0 && c < t.n_chrom && rcnt_fragment(mode, pos[i], tlen[i], flag_mapq[i], min_mapq, read_width, fs, fe)) {
        const int32_t co = t.chrom_off[c], ce = t.chrom_off[c + 1];
        int32_t a = co, b = ce;                       // first position in [co, ce) with end >= fs
        while (a < b) {
          const int32_t m = a + ((b - a) >> 1);
          if ((int64_t)t.ends[m] < fs) a = m + 1; else b = m;
        }
        if (a < ce) slotA = a;
        a = co; b = ce;                               // first position in [co, ce) with start > fe
        while (a < b) {
          const int32_t m = a + ((b - a) >> 1);
          if ((int64_t)t.starts[m] <= fe) a = m + 1; else b = m;
        }
        if (a < ce) slotB = a;
      }
    }
    rcnt_merged_add(histA, slotA);
    rcnt_merged_add(histB, slotB);
  }
}

// inclusive scan of h[lo, hi) in place by one workgroup, kRcntFinishBlock values a step with the running total carried along
__device__ __forceinline__ void rcnt_scan(unsigned int* __restrict__ h, int32_t lo, int32_t hi, unsigned int* sh)
{
  const int t = threadIdx.x;
  unsigned int carry = 0;
  for (int32_t p0 = lo; p0 < hi; p0 += kRcntFinishBlock) {
    const int32_t p = p0 + t;
    const unsigned int v = p < hi ? h[p] : 0u;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kRcntFinishBlock; d <<= 1) {
      const unsigned int add = t >= d ? sh[t - d] : 0u;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    if (p < hi) h[p] = carry + sh[t];
    carry += sh[kRcntFinishBlock - 1];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kRcntFinishBlock)
k_rcnt_finish(RcntTable t, unsigned int* __restrict__ histA, unsigned int* __restrict__ histB, int32_t* __restrict__ counts)
{
  __shared__ unsigned int sh[kRcntFinishBlock];
  const int32_t co = t.chrom_off[blockIdx.x], ce = t.chrom_off[blockIdx.x + 1];
  rcnt_scan(histA, co, ce, sh);
  rcnt_scan(histB, co, ce, sh);
  __syncthreads();                                    // both scans of this chromosome are complete and visible to the workgroup
  for (int32_t p = co + (int32_t)threadIdx.x; p < ce; p += kRcntFinishBlock) {
    const int32_t e = t.end_exon[p];
    counts[e] += (int32_t)(histA[p] - histB[t.start_rank[e]]);
  }
  __syncthreads();
  for (int32_t p = co + (int32_t)threadIdx.x; p < ce; p += kRcntFinishBlock) { histA[p] = 0u; histB[p] = 0u; }
}

// counts [n_columns][n] -> out [n][n_columns], the exon-major form (what the PCA correction and the reference-set selection read); 32 x 32 tiles
// through LDS so that both sides are coalesced
__global__ void __launch_bounds__(256)
k_rcnt_transpose(const int32_t* __restrict__ in, int64_t n, int32_t n_columns, int32_t* __restrict__ out)
{
  __shared__ int32_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * 32;
  const int32_t c0 = (int32_t)blockIdx.y * 32;
  for (int k = ty; k < 32; k += 8) {
    const int64_t e = e0 + tx;
    const int32_t c = c0 + k;
    tile[k][tx] = (e < n && c < n_columns) ? in[(size_t)c * (size_t)n + (size_t)e] : 0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int64_t e = e0 + k;
    const int32_t c = c0 + tx;
    if (e < n && c < n_columns) out[(size_t)e * (size_t)n_columns + (size_t)c] = tile[tx][k];
  }
}

struct RcntSet {               // one staging set: a chunk's four arrays + the refID table, pinned and on the device
  PinBuf<char> pin;
  DevBuf<char> dev;
  Event up, k0, k1;            // upload complete; around the chunk's kernel
  bool busy = false;           // a kernel reading this set has been launched and its time not yet collected
};

}  // namespace

struct ed_readcount {
  int device = 0;
  int64_t n = 0;
  int32_t n_chrom = 0, n_columns = 0;
  int32_t pending = -1;        // the column with chunks added and not finished, or -1
  int64_t n_sub = 0;           // staged uploads so far (their parity picks the set)
  double bin_ms = 0.0, finish_ms = 0.0;
  bool finish_timed = false;
  DevBuf<char> d_table;        // ONE allocation: ends, starts, end_exon, start_rank (int32 [n] each), chrom_off (int32 [n_chrom + 1])
  RcntTable table{};
  DevBuf<unsigned int> d_hist; // histA [n], histB [n]
  DevBuf<int32_t> d_counts;    // [n_columns][n]
  RcntSet set[2];
  Event f0, f1;                // around k_rcnt_finish
  DevBuf<int32_t> d_r2c;       // ed_readcount_add_device: the refID table
  Event dev_ready;             // ... and the caller's stream at the time of the call
  Stream copy, stream;         // (declared last: they go first, after ed_readcount_destroy has waited for them)
};

static size_t rcnt_up(size_t b) { return (b + 255) & ~(size_t)255; }

// the time of a set's finished kernel into the total; the caller has waited for k1
static int rcnt_collect(ed_readcount* a, RcntSet& s)
{
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
  a->bin_ms += (double)ms;
  s.busy = false;
  return ED_OK;
}

// everything queued on the object is complete on return, and its kernels' times are in the totals
static int rcnt_drain(ed_readcount* a)
{
  HIP_TRY(hipStreamSynchronize(a->copy));
  HIP_TRY(hipStreamSynchronize(a->stream));
  for (RcntSet& s : a->set)
    if (s.busy) { if (int rc = rcnt_collect(a, s)) return rc; }
  if (a->finish_timed) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a->f0, a->f1));
    a->finish_ms += (double)ms;
    a->finish_timed = false;
  }
  return ED_OK;
}

ED_EXPORT void ed_readcount_destroy(ed_readcount* a)
{
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->copy) (void)hipStreamSynchronize(a->copy);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  delete a;
}

// out = {threads of a workgroup of k_rcnt_bin, records a workgroup takes, bins of a workgroup-private window (0: none was built), values of one
// step of the finish scan}: what a test needs to place its shapes on the edges
ED_EXPORT int ed_readcount_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_readcount_geometry: NULL output");
  out[0] = kRcntBlock; out[1] = kRcntPerGroup; out[2] = 0; out[3] = kRcntFinishBlock;
  return ED_OK;
}
ED_CATCH("ed_readcount_geometry")

ED_EXPORT int ed_bam_scan_records(const uint8_t* buf, int64_t n_bytes, int64_t cap, int32_t* refid, int32_t* pos, int32_t* tlen,
                                  uint32_t* flag_mapq, int64_t* n_records, int64_t* bytes_consumed)
try {
  if (n_bytes < 0 || cap < 0 || !n_records || !bytes_consumed || (n_bytes > 0 && !buf) || (cap > 0 && (!refid || !pos || !tlen || !flag_mapq)))
    return ed_fail(ED_ERR_INVALID, "ed_bam_scan_records: bad arguments");
  int64_t bad_off = 0;
  int32_t bad = 0;
  if (edbam::scan_records(buf, n_bytes, cap, refid, pos, tlen, flag_mapq, n_records, bytes_consumed, &bad_off, &bad) != edbam::kScanOk)
    return ed_fail(ED_ERR_INVALID, "ed_bam_scan_records: record %lld at byte %lld has block_size %d (32 .. %d wanted): not a BAM record stream, or a "
                   "corrupt one", (long long)*n_records, (long long)bad_off, bad, edbam::kMaxBlock);
  return ED_OK;
}
ED_CATCH("ed_bam_scan_records")

ED_EXPORT int ed_readcount_create(ed_readcount** rc_out, int device, int64_t n, int32_t n_chrom, const int32_t* chrom, const int32_t* start,
                                  const int32_t* end, int32_t n_columns)
try {
  if (!rc_out || n < 0 || n_chrom < 0 || n_columns < 1 || (n > 0 && (!chrom || !start || !end)))
    return ed_fail(ED_ERR_INVALID, "ed_readcount_create: bad arguments");
  if (n > 2147483647LL - kRcntFinishBlock) return ed_fail(ED_ERR_INVALID, "ed_readcount_create: too many exons (positions are int32)");
  for (int64_t i = 0; i < n; ++i) {
    if (chrom[i] < 0 || chrom[i] >= n_chrom)
      return ed_fail(ED_ERR_INVALID, "ed_readcount_create: exon %lld has chromosome id %d outside 0 .. %d", (long long)i, chrom[i], n_chrom - 1);
    if (start[i] < 1 || end[i] < start[i])
      return ed_fail(ED_ERR_INVALID, "ed_readcount_create: exon %lld has start %d, end %d (1 <= start <= end wanted)", (long long)i, start[i], end[i]);
  }
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(device));
  // counting sort by chromosome, then the two orders within each
  std::vector<int32_t> off((size_t)n_chrom + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++off[(size_t)chrom[i] + 1];
  for (int32_t c = 0; c < n_chrom; ++c) off[(size_t)c + 1] += off[c];
  std::vector<int32_t> by_end((size_t)n), by_start;
  {
    std::vector<int32_t> at(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; ++i) by_end[(size_t)at[chrom[i]]++] = (int32_t)i;
  }
  by_start = by_end;
  for (int32_t c = 0; c < n_chrom; ++c) {
    std::stable_sort(by_end.begin() + off[c], by_end.begin() + off[(size_t)c + 1], [end](int32_t a, int32_t b) { return end[a] < end[b]; });
    std::stable_sort(by_start.begin() + off[c], by_start.begin() + off[(size_t)c + 1], [start](int32_t a, int32_t b) { return start[a] < start[b]; });
  }
  const size_t arr = rcnt_up((size_t)std::max<int64_t>(n, 1) * 4), bytes = 4 * arr + rcnt_up(((size_t)n_chrom + 1) * 4);
  std::vector<char> img(bytes, 0);
  int32_t* h_ends = (int32_t*)img.data();
  int32_t* h_starts = (int32_t*)(img.data() + arr);
  int32_t* h_end_exon = (int32_t*)(img.data() + 2 * arr);
  int32_t* h_start_rank = (int32_t*)(img.data() + 3 * arr);
  int32_t* h_off = (int32_t*)(img.data() + 4 * arr);
  for (int64_t p = 0; p < n; ++p) {
    h_ends[p] = end[by_end[(size_t)p]];
    h_end_exon[p] = by_end[(size_t)p];
    h_starts[p] = start[by_start[(size_t)p]];
    h_start_rank[by_start[(size_t)p]] = (int32_t)p;
  }
  for (int32_t c = 0; c <= n_chrom; ++c) h_off[c] = off[c];
  ed_readcount* a = new (std::nothrow) ed_readcount;
  if (!a) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  struct Guard { ed_readcount* a; ~Guard() { if (a) ed_readcount_destroy(a); } } guard{a};   // released on success only
  a->device = device; a->n = n; a->n_chrom = n_chrom; a->n_columns = n_columns;
  const size_t hist_bytes = 2 * (size_t)std::max<int64_t>(n, 1) * 4, count_bytes = (size_t)n_columns * (size_t)std::max<int64_t>(n, 1) * 4;
  if (a->d_table.alloc(bytes) != hipSuccess || a->d_hist.alloc(hist_bytes) != hipSuccess || a->d_counts.alloc(count_bytes) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_readcount_create: device allocation of %zu bytes failed", bytes + hist_bytes + count_bytes);
  for (Stream* s : {&a->stream, &a->copy}) {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s->reset(st);
  }
  for (RcntSet& s : a->set) {
    HIP_TRY(s.up.create(hipEventDisableTiming));
    HIP_TRY(s.k0.create());
    HIP_TRY(s.k1.create());
  }
  HIP_TRY(a->f0.create());
  HIP_TRY(a->f1.create());
  HIP_TRY(hipMemcpyAsync(a->d_table, img.data(), bytes, hipMemcpyHostToDevice, a->stream));
  HIP_TRY(hipMemsetAsync(a->d_hist, 0, hist_bytes, a->stream));
  HIP_TRY(hipMemsetAsync(a->d_counts, 0, count_bytes, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  char* d = a->d_table;
  a->table.ends = (const int32_t*)d;
  a->table.starts = (const int32_t*)(d + arr);
  a->table.end_exon = (const int32_t*)(d + 2 * arr);
  a->table.start_rank = (const int32_t*)(d + 3 * arr);
  a->table.chrom_off = (const int32_t*)(d + 4 * arr);
  a->table.n_chrom = n_chrom;
  guard.a = nullptr;
  *rc_out = a;
  return ED_OK;
}
ED_CATCH("ed_readcount_create")

ED_EXPORT int ed_readcount_add(ed_readcount* a, int32_t column, int mode, int64_t n_records, const int32_t* refid, const int32_t* pos,
                               const int32_t* tlen, const uint32_t* flag_mapq, int32_t n_ref, const int32_t* ref_to_chrom, int32_t min_mapq,
                               int32_t read_width)
try {
  if (!a || n_records < 0 || n_ref < 0 || (n_records > 0 && (!refid || !pos || !tlen || !flag_mapq)) || (n_ref > 0 && !ref_to_chrom))
    return ed_fail(ED_ERR_INVALID, "ed_readcount_add: bad arguments");
  if (column < 0 || column >= a->n_columns)
    return ed_fail(ED_ERR_INVALID, "ed_readcount_add: column %d outside 0 .. %d", column, a->n_columns - 1);
  if (mode != 0 && mode != 1) return ed_fail(ED_ERR_INVALID, "ed_readcount_add: mode %d (0 = getBamCounts' rule, 1 = everted reads)", mode);
  if (read_width < 0) return ed_fail(ED_ERR_INVALID, "ed_readcount_add: read_width %d < 0", read_width);
  for (int32_t r = 0; r < n_ref; ++r)
    if (ref_to_chrom[r] < -1 || ref_to_chrom[r] >= a->n_chrom)
      return ed_fail(ED_ERR_INVALID, "ed_readcount_add: ref_to_chrom[%d] = %d outside -1 .. %d", r, ref_to_chrom[r], a->n_chrom - 1);
  if (a->pending >= 0 && a->pending != column)
    return ed_fail(ED_ERR_STATE, "ed_readcount_add: column %d has chunks added and is not finished (ed_readcount_finish); the histograms serve one "
                   "column at a time", a->pending);
  HIP_TRY(hipSetDevice(a->device));
  if (n_records == 0 || a->n == 0 || n_ref == 0) return ED_OK;
  a->pending = column;
  unsigned int* histA = a->d_hist;
  unsigned int* histB = histA + a->n;
  for (int64_t r0 = 0; r0 < n_records; r0 += kRcntChunk) {
    const int64_t m = std::min<int64_t>(kRcntChunk, n_records - r0);
    RcntSet& s = a->set[a->n_sub & 1];
    if (s.busy) {                                       // the kernel that read this set two uploads ago: its arrays are free once it is done
      HIP_TRY(hipEventSynchronize(s.k1));
      if (int rc = rcnt_collect(a, s)) return rc;
    }
    const size_t arr = rcnt_up((size_t)m * 4), need = 4 * arr + rcnt_up((size_t)n_ref * 4);
    if (s.pin.reserve(need) != hipSuccess || s.dev.reserve(need) != hipSuccess)
      return ed_fail(ED_ERR_NOMEM, "ed_readcount_add: staging allocation of %zu bytes failed", need);
    char* h = s.pin;
    std::memcpy(h, refid + r0, (size_t)m * 4);
    std::memcpy(h + arr, pos + r0, (size_t)m * 4);
    std::memcpy(h + 2 * arr, tlen + r0, (size_t)m * 4);
    std::memcpy(h + 3 * arr, flag_mapq + r0, (size_t)m * 4);
    std::memcpy(h + 4 * arr, ref_to_chrom, (size_t)n_ref * 4);
    // the upload goes on the copy stream, under the kernel of the other set; the kernel waits for it
    HIP_TRY(hipMemcpyAsync(s.dev, s.pin, need, hipMemcpyHostToDevice, a->copy));
    HIP_TRY(hipEventRecord(s.up, a->copy));
    HIP_TRY(hipStreamWaitEvent(a->stream, s.up, 0));
    char* d = s.dev;
    const unsigned int grid = (unsigned int)((m + kRcntPerGroup - 1) / kRcntPerGroup);
    HIP_TRY(hipEventRecord(s.k0, a->stream));
    hipLaunchKernelGGL(k_rcnt_bin, dim3(grid), dim3(kRcntBlock), 0, a->stream, a->table, (const int32_t*)d, (const int32_t*)(d + arr),
                       (const int32_t*)(d + 2 * arr), (const uint32_t*)(d + 3 * arr), m, (const int32_t*)(d + 4 * arr), n_ref, mode, min_mapq,
                       read_width, histA, histB);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.k1, a->stream));
    s.busy = true;
    ++a->n_sub;
  }
  return ED_OK;
}
ED_CATCH("ed_readcount_add")

// ed_readcount_add with the four arrays already on the DEVICE, ordered behind ready_stream (what the caller queued there before the call is complete
// before the arrays are read).  The same kernel, the same refusals, the same one-column-at-a-time state; the arrays have been read when it returns.
ED_EXPORT int ed_readcount_add_device(ed_readcount* a, int32_t column, int mode, int64_t n_records, const int32_t* d_refid, const int32_t* d_pos,
                                      const int32_t* d_tlen, const uint32_t* d_flag_mapq, int32_t n_ref, const int32_t* ref_to_chrom, int32_t min_mapq,
                                      int32_t read_width, void* ready_stream)
try {
  if (!a || n_records < 0 || n_ref < 0 || (n_records > 0 && (!d_refid || !d_pos || !d_tlen || !d_flag_mapq)) || (n_ref > 0 && !ref_to_chrom))
    return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: bad arguments");
  if (column < 0 || column >= a->n_columns)
    return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: column %d outside 0 .. %d", column, a->n_columns - 1);
  if (mode != 0 && mode != 1) return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: mode %d (0 = getBamCounts' rule, 1 = everted reads)", mode);
  if (read_width < 0) return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: read_width %d < 0", read_width);
  for (int32_t r = 0; r < n_ref; ++r)
    if (ref_to_chrom[r] < -1 || ref_to_chrom[r] >= a->n_chrom)
      return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: ref_to_chrom[%d] = %d outside -1 .. %d", r, ref_to_chrom[r], a->n_chrom - 1);
  if (a->pending >= 0 && a->pending != column)
    return ed_fail(ED_ERR_STATE, "ed_readcount_add_device: column %d has chunks added and is not finished (ed_readcount_finish); the histograms serve "
                   "one column at a time", a->pending);
  HIP_TRY(hipSetDevice(a->device));
  if (n_records == 0 || a->n == 0 || n_ref == 0) return ED_OK;
  if (n_records > (int64_t)2147483647 * kRcntPerGroup) return ed_fail(ED_ERR_INVALID, "ed_readcount_add_device: too many records for one launch");
  if (a->d_r2c.reserve((size_t)n_ref * 4) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "ed_readcount_add_device: device allocation failed");
  if (!a->dev_ready) HIP_TRY(a->dev_ready.create(hipEventDisableTiming));
  a->pending = column;
  HIP_TRY(hipMemcpyAsync(a->d_r2c.get(), ref_to_chrom, (size_t)n_ref * 4, hipMemcpyHostToDevice, a->stream));
  HIP_TRY(hipEventRecord(a->dev_ready, (hipStream_t)ready_stream));
  HIP_TRY(hipStreamWaitEvent(a->stream, a->dev_ready, 0));
  unsigned int* histA = a->d_hist;
  hipLaunchKernelGGL(k_rcnt_bin, dim3((unsigned int)((n_records + kRcntPerGroup - 1) / kRcntPerGroup)), dim3(kRcntBlock), 0, a->stream, a->table, d_refid,
                     d_pos, d_tlen, d_flag_mapq, n_records, (const int32_t*)a->d_r2c.get(), n_ref, mode, min_mapq, read_width, histA, histA + a->n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(a->stream));             // the caller's arrays (a bamdev batch's) are free again
  return ED_OK;
}
ED_CATCH("ed_readcount_add_device")

ED_EXPORT int ed_readcount_finish(ed_readcount* a, int32_t column)
try {
  if (!a) return ed_fail(ED_ERR_INVALID, "ed_readcount_finish: NULL object");
  if (column < 0 || column >= a->n_columns)
    return ed_fail(ED_ERR_INVALID, "ed_readcount_finish: column %d outside 0 .. %d", column, a->n_columns - 1);
  if (a->pending >= 0 && a->pending != column)
    return ed_fail(ED_ERR_STATE, "ed_readcount_finish: the chunks added belong to column %d, not %d", a->pending, column);
  if (a->pending < 0) return ED_OK;                     // nothing was added: the histograms are clear and the column stands
  HIP_TRY(hipSetDevice(a->device));
  if (a->finish_timed) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(a->f1));
    HIP_TRY(hipEventElapsedTime(&ms, a->f0, a->f1));
    a->finish_ms += (double)ms;
    a->finish_timed = false;
  }
  unsigned int* histA = a->d_hist;
  HIP_TRY(hipEventRecord(a->f0, a->stream));
  hipLaunchKernelGGL(k_rcnt_finish, dim3((unsigned int)a->n_chrom), dim3(kRcntFinishBlock), 0, a->stream, a->table, histA, histA + a->n,
                     a->d_counts.get() + (size_t)column * (size_t)a->n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(a->f1, a->stream));
  a->finish_timed = true;
  a->pending = -1;
  return ED_OK;
}
ED_CATCH("ed_readcount_finish")

ED_EXPORT int ed_readcount_copy(ed_readcount* a, int32_t column0, int32_t n_columns, int32_t* out)
try {
  if (!a || column0 < 0 || n_columns < 0 || (int64_t)column0 + n_columns > a->n_columns || (n_columns > 0 && !out))
    return ed_fail(ED_ERR_INVALID, "ed_readcount_copy: bad arguments");
  if (a->pending >= column0 && a->pending < column0 + n_columns)
    return ed_fail(ED_ERR_STATE, "ed_readcount_copy: column %d has chunks added and is not finished (ed_readcount_finish)", a->pending);
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = rcnt_drain(a)) return rc;
  if (n_columns == 0 || a->n == 0) return ED_OK;
  HIP_TRY(hipMemcpy(out, a->d_counts.get() + (size_t)column0 * (size_t)a->n, (size_t)n_columns * (size_t)a->n * 4, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_readcount_copy")

// the matrix itself; what has been queued on the object is complete when this returns (NULL, with ed_last_error(), if waiting for it failed)
ED_EXPORT void* ed_readcount_device_counts(ed_readcount* a)
{
  if (!a) return nullptr;
  if (hipSetDevice(a->device) != hipSuccess || rcnt_drain(a) != ED_OK) return nullptr;
  return a->d_counts.get();
}

// d_out: DEVICE int32 [n_exons][n_columns], the caller's; complete when this returns
ED_EXPORT int ed_readcount_copy_exon_major(ed_readcount* a, int32_t* d_out)
try {
  if (!a || !d_out) return ed_fail(ED_ERR_INVALID, "ed_readcount_copy_exon_major: NULL argument");
  if (a->n_columns > 32 * 65535) return ed_fail(ED_ERR_INVALID, "ed_readcount_copy_exon_major: at most %d columns", 32 * 65535);
  if (a->pending >= 0)
    return ed_fail(ED_ERR_STATE, "ed_readcount_copy_exon_major: column %d has chunks added and is not finished (ed_readcount_finish)", a->pending);
  HIP_TRY(hipSetDevice(a->device));
  if (a->n > 0) {
    hipLaunchKernelGGL(k_rcnt_transpose, dim3((unsigned int)((a->n + 31) / 32), (unsigned int)((a->n_columns + 31) / 32)), dim3(256), 0, a->stream,
                       (const int32_t*)a->d_counts.get(), a->n, a->n_columns, d_out);
    HIP_TRY(hipGetLastError());
  }
  return rcnt_drain(a);
}
ED_CATCH("ed_readcount_copy_exon_major")

ED_EXPORT int ed_readcount_kernel_ms(ed_readcount* a, double* bin_ms, double* finish_ms)
try {
  if (!a || !bin_ms || !finish_ms) return ed_fail(ED_ERR_INVALID, "ed_readcount_kernel_ms: NULL argument");
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = rcnt_drain(a)) return rc;
  *bin_ms = a->bin_ms; *finish_ms = a->finish_ms;
  return ED_OK;
}
ED_CATCH("ed_readcount_kernel_ms")
