// edgc.inc -- letter classes in byte ranges of a file: the GC column of getBamCounts (referenceFasta, R/countBamInGranges.R:333-344), on the device
// (included at the end of edcore.hip).  DESIGN 4.27.
//
// A target is a range [first, last_excl) of FILE byte addresses -- the caller's business (fasta.py: a FASTA record's offset and line geometry);
// nothing here knows about FASTA.  Per target two sums over the bytes of its range, the byte folded to lower case with | 0x20:
//   gc    #{'c', 'g'}
//   atgc  #{'a', 'c', 'g', 't'}
// (x | 0x20) == v for a v with bit 5 set holds for x == v and x == v ^ 0x20 only, so exactly the eight letters AaCcGgTt count.  Everything else
// -- N, the IUPAC codes, line ends, any other byte -- counts in neither: letterFrequency(x, "GC") / letterFrequency(x, "ATGC") on the DNAString.
//
// The file arrives in chunks (ed_gc_add): bytes [file_offset, file_offset + n_bytes) and the ranges that touch them.  k_gc_count clips every range
// to the chunk and ADDS what it finds to the target's two sums, so a target cut by chunk borders is the sum of its pieces.  Integer adds only: the
// result is the same bits whatever the cuts, the order of the ranges or the launch geometry.
//
//   k_gc_count   a wavefront per (range, segment): the clipped range in segments of kGcSegment bytes.  A lane loads 16 bytes at a 16-byte aligned
//                address a step (64 lanes: 1 KiB), the bytes of the first and the last load that lie outside the segment are masked; the four
//                classes are matched a dword at a time (an exact zero-byte test, no carry between bytes), counted with popcount, summed over
//                the wavefront, and lane 0 adds the two sums to the target (int32 atomics, nothing else).  No LDS, no scratch.

namespace {

constexpr int kGcBlock = 256;                                // threads of k_gc_count: four wavefronts, a (range, segment) each
constexpr int kGcLaneBytes = 16;                             // bytes a lane loads a step
constexpr int kGcStep = 64 * kGcLaneBytes;                   // bytes a wavefront takes a step
constexpr int kGcSegment = 2 * kGcStep;                      // bytes of a segment: a wavefront's share of a range
constexpr int64_t kGcPiece = (int64_t)1 << 26;               // bytes of one staged upload at the most (64 MiB a staging set)

// bit 7 of every byte of a dword whose index is below n (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint32_t gc_low_bytes(int n)
{
  return n <= 0 ? 0u : n >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * n)) - 1u));
}

// bit 7 of every byte of z that is zero; exact: (z & 0x7f) + 0x7f stays inside its byte
__device__ __forceinline__ uint32_t gc_zero_bytes(uint32_t z)
{
  return ~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u;
}

// first / last_excl / target [n_ranges]: the ranges with at least one byte in the chunk; unit_off [n_ranges + 1]: the exclusive scan of their segment
// counts AFTER clipping to [chunk_lo, chunk_hi).  bytes[0] is the file's byte at address bytes_addr (a multiple of 16 below the first byte any range
// reads, the buffer 16-byte aligned and a multiple of 16 long).
__global__ void __launch_bounds__(kGcBlock)
k_gc_count(const uint8_t* __restrict__ bytes, int64_t bytes_addr, int64_t chunk_lo, int64_t chunk_hi, int32_t n_ranges,
           const int64_t* __restrict__ first, const int64_t* __restrict__ last_excl, const int32_t* __restrict__ target,
           const int32_t* __restrict__ unit_off, int32_t n_units, int32_t* __restrict__ gc, int32_t* __restrict__ atgc)
{
  const int lane = threadIdx.x & 63;
  const int32_t unit = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * (kGcBlock / 64) + (threadIdx.x >> 6)));
  if (unit >= n_units) return;
  int32_t a = 0, b = n_ranges;                       // the last range with unit_off <= unit (ranges without a segment share their successor's offset)
  while (b - a > 1) {
    const int32_t m = a + ((b - a) >> 1);
    if (unit_off[m] <= unit) a = m; else b = m;
  }
  const int64_t f = first[a], l = last_excl[a];
  const int64_t lo = f > chunk_lo ? f : chunk_lo, hi = l < chunk_hi ? l : chunk_hi;
  const int64_t s_lo = lo + (int64_t)(unit - unit_off[a]) * kGcSegment;
  const int64_t s_hi = s_lo + kGcSegment < hi ? s_lo + kGcSegment : hi;
  if (s_lo >= s_hi) return;                          // (cannot happen with a unit_off made from the same clipping)
  const int64_t rel_lo = s_lo - bytes_addr, rel_hi = s_hi - bytes_addr;
  const int64_t base = (rel_lo & ~(int64_t)(kGcLaneBytes - 1)) + (int64_t)lane * kGcLaneBytes;
  int32_t n_gc = 0, n_at = 0;
  // the first load starts at most 15 bytes before the segment, so kGcSegment / kGcStep + 1 steps cover it
#pragma unroll
  for (int k = 0; k <= kGcSegment / kGcStep; ++k) {
    const int64_t p = base + (int64_t)k * kGcStep;
    if (p < rel_hi) {                                // p + 16 > rel_lo holds for every lane: p >= rel_lo - 15
      const uint4 v = *reinterpret_cast<const uint4*>(bytes + p);
      const int from = rel_lo > p ? (int)(rel_lo - p) : 0, to = rel_hi - p < kGcLaneBytes ? (int)(rel_hi - p) : kGcLaneBytes;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t valid = gc_low_bytes(to - 4 * d) & ~gc_low_bytes(from - 4 * d);
        const uint32_t y = w[d] | 0x20202020u;
        const uint32_t m_gc = gc_zero_bytes(y ^ 0x63636363u) | gc_zero_bytes(y ^ 0x67676767u);
        const uint32_t m_at = gc_zero_bytes(y ^ 0x61616161u) | gc_zero_bytes(y ^ 0x74747474u);
        n_gc += __popc(m_gc & valid);
        n_at += __popc(m_at & valid);
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    n_gc += __shfl_xor(n_gc, d, 64);
    n_at += __shfl_xor(n_at, d, 64);
  }
  if (lane == 0) {
    const int32_t t = target[a];
    if (n_gc) atomicAdd(&gc[t], n_gc);
    if (n_gc + n_at) atomicAdd(&atgc[t], n_gc + n_at);
  }
}

struct GcSet {                 // one staging set: a piece's bytes and its ranges, pinned and on the device
  PinBuf<char> pin;
  DevBuf<char> dev;
  Event up, k0, k1;            // upload complete; around the piece's kernel
  bool busy = false;           // a kernel reading this set has been launched and its time not yet collected
};

}  // namespace

struct ed_gc {
  int device = 0;
  int64_t n = 0;               // targets
  int64_t n_sub = 0;           // staged uploads so far (their parity picks the set)
  double kernel_ms = 0.0;
  DevBuf<int32_t> d_sums;      // gc [n], atgc [n]
  GcSet set[2];
  std::vector<int64_t> h_first, h_last;   // the ranges of a piece that have a byte in it, and their segments
  std::vector<int32_t> h_target, h_off;
  Stream copy, stream;         // (declared last: they go first, after ed_gc_destroy has waited for them)
};

static size_t gc_up(size_t b) { return (b + 255) & ~(size_t)255; }

static int gc_collect(ed_gc* a, GcSet& s)
{
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
  a->kernel_ms += (double)ms;
  s.busy = false;
  return ED_OK;
}

// everything queued on the object is complete on return, and its kernels' times are in the total
static int gc_drain(ed_gc* a)
{
  HIP_TRY(hipStreamSynchronize(a->copy));
  HIP_TRY(hipStreamSynchronize(a->stream));
  for (GcSet& s : a->set)
    if (s.busy) { if (int rc = gc_collect(a, s)) return rc; }
  return ED_OK;
}

// one piece of at most kGcPiece bytes: the ranges with a byte in it, staged with the bytes they span, and one launch
static int gc_add_piece(ed_gc* a, const uint8_t* bytes, int64_t n_bytes, int64_t file_offset, int64_t n_ranges, const int64_t* first,
                        const int64_t* last_excl, const int64_t* target)
{
  const int64_t c_lo = file_offset, c_hi = file_offset + n_bytes;
  a->h_first.clear(); a->h_last.clear(); a->h_target.clear(); a->h_off.clear();
  int64_t units = 0, b_lo = c_hi, b_hi = c_lo;
  for (int64_t r = 0; r < n_ranges; ++r) {
    const int64_t lo = std::max(first[r], c_lo), hi = std::min(last_excl[r], c_hi);
    if (lo >= hi) continue;
    a->h_first.push_back(first[r]); a->h_last.push_back(last_excl[r]); a->h_target.push_back((int32_t)target[r]);
    a->h_off.push_back((int32_t)units);
    units += (hi - lo + kGcSegment - 1) / kGcSegment;
    if (units > 2147483647LL - kGcBlock) return ed_fail(ED_ERR_INVALID, "ed_gc_add: too many (range, segment) pairs for one launch");
    b_lo = std::min(b_lo, lo); b_hi = std::max(b_hi, hi);
  }
  if (units == 0) return ED_OK;
  a->h_off.push_back((int32_t)units);
  const size_t m = a->h_first.size();
  b_lo = c_lo + ((b_lo - c_lo) & ~(int64_t)(kGcLaneBytes - 1));      // the bytes any range reads, from a multiple of 16 within the piece
  const size_t span = (size_t)(b_hi - b_lo), o_first = gc_up(span + kGcLaneBytes), o_last = o_first + gc_up(m * 8), o_target = o_last + gc_up(m * 8),
               o_off = o_target + gc_up(m * 4), need = o_off + gc_up((m + 1) * 4);
  GcSet& s = a->set[a->n_sub & 1];
  if (s.busy) {                                         // the kernel that read this set two uploads ago: its arrays are free once it is done
    HIP_TRY(hipEventSynchronize(s.k1));
    if (int rc = gc_collect(a, s)) return rc;
  }
  if (s.pin.reserve(need) != hipSuccess || s.dev.reserve(need) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_gc_add: staging allocation of %zu bytes failed", need);
  char* h = s.pin;
  std::memcpy(h, bytes + (b_lo - c_lo), span);
  std::memset(h + span, 0, o_first - span);             // the tail of the last 16-byte load
  std::memcpy(h + o_first, a->h_first.data(), m * 8);
  std::memcpy(h + o_last, a->h_last.data(), m * 8);
  std::memcpy(h + o_target, a->h_target.data(), m * 4);
  std::memcpy(h + o_off, a->h_off.data(), (m + 1) * 4);
  // the upload goes on the copy stream, under the kernel of the other set; the kernel waits for it
  HIP_TRY(hipMemcpyAsync(s.dev, s.pin, need, hipMemcpyHostToDevice, a->copy));
  HIP_TRY(hipEventRecord(s.up, a->copy));
  HIP_TRY(hipStreamWaitEvent(a->stream, s.up, 0));
  char* d = s.dev;
  const unsigned int grid = (unsigned int)((units + kGcBlock / 64 - 1) / (kGcBlock / 64));
  HIP_TRY(hipEventRecord(s.k0, a->stream));
  hipLaunchKernelGGL(k_gc_count, dim3(grid), dim3(kGcBlock), 0, a->stream, (const uint8_t*)d, b_lo, c_lo, c_hi, (int32_t)m,
                     (const int64_t*)(d + o_first), (const int64_t*)(d + o_last), (const int32_t*)(d + o_target), (const int32_t*)(d + o_off),
                     (int32_t)units, a->d_sums.get(), a->d_sums.get() + a->n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.k1, a->stream));
  s.busy = true;
  ++a->n_sub;
  return ED_OK;
}

ED_EXPORT void ed_gc_destroy(ed_gc* a)
{
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->copy) (void)hipStreamSynchronize(a->copy);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  delete a;
}

// out = {threads of a workgroup of k_gc_count, bytes of a segment (a wavefront's share of a range), bytes a wavefront takes a step, bytes a lane
// loads a step}: what a test needs to place its shapes on the edges
ED_EXPORT int ed_gc_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_gc_geometry: NULL output");
  out[0] = kGcBlock; out[1] = kGcSegment; out[2] = kGcStep; out[3] = kGcLaneBytes;
  return ED_OK;
}
ED_CATCH("ed_gc_geometry")

ED_EXPORT int ed_gc_create(ed_gc** gc_out, int device, int64_t n_targets)
try {
  if (!gc_out || n_targets < 0) return ed_fail(ED_ERR_INVALID, "ed_gc_create: bad arguments");
  if (n_targets > 2147483647LL) return ed_fail(ED_ERR_INVALID, "ed_gc_create: too many targets (their index is int32)");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(device));
  ed_gc* a = new (std::nothrow) ed_gc;
  if (!a) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  struct Guard { ed_gc* a; ~Guard() { if (a) ed_gc_destroy(a); } } guard{a};   // released on success only
  a->device = device; a->n = n_targets;
  const size_t sum_bytes = 2 * (size_t)std::max<int64_t>(n_targets, 1) * 4;
  if (a->d_sums.alloc(sum_bytes) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "ed_gc_create: device allocation of %zu bytes failed", sum_bytes);
  for (Stream* s : {&a->stream, &a->copy}) {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s->reset(st);
  }
  for (GcSet& s : a->set) {
    HIP_TRY(s.up.create(hipEventDisableTiming));
    HIP_TRY(s.k0.create());
    HIP_TRY(s.k1.create());
  }
  HIP_TRY(hipMemsetAsync(a->d_sums, 0, sum_bytes, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  guard.a = nullptr;
  *gc_out = a;
  return ED_OK;
}
ED_CATCH("ed_gc_create")

ED_EXPORT int ed_gc_add(ed_gc* a, const uint8_t* bytes, int64_t n_bytes, int64_t file_offset, int64_t n_ranges, const int64_t* first,
                        const int64_t* last_excl, const int64_t* target)
try {
  if (!a || n_bytes < 0 || n_ranges < 0 || file_offset < 0 || (n_bytes > 0 && !bytes) || (n_ranges > 0 && (!first || !last_excl || !target)))
    return ed_fail(ED_ERR_INVALID, "ed_gc_add: bad arguments (NULL array, or a negative size or offset)");
  if (file_offset > INT64_MAX - n_bytes) return ed_fail(ED_ERR_INVALID, "ed_gc_add: file_offset + n_bytes overflows");
  for (int64_t r = 0; r < n_ranges; ++r) {
    if (target[r] < 0 || target[r] >= a->n)
      return ed_fail(ED_ERR_INVALID, "ed_gc_add: range %lld has target %lld outside 0 .. %lld", (long long)r, (long long)target[r], (long long)a->n - 1);
    if (first[r] > last_excl[r])
      return ed_fail(ED_ERR_INVALID, "ed_gc_add: range %lld is [%lld, %lld): first <= last_excl wanted", (long long)r, (long long)first[r],
                     (long long)last_excl[r]);
  }
  HIP_TRY(hipSetDevice(a->device));
  for (int64_t p = 0; p < n_bytes; p += kGcPiece) {
    const int64_t m = std::min<int64_t>(kGcPiece, n_bytes - p);
    if (int rc = gc_add_piece(a, bytes + p, m, file_offset + p, n_ranges, first, last_excl, target)) return rc;
  }
  return ED_OK;
}
ED_CATCH("ed_gc_add")

ED_EXPORT int ed_gc_copy(ed_gc* a, int32_t* gc, int32_t* atgc)
try {
  if (!a || (a->n > 0 && (!gc || !atgc))) return ed_fail(ED_ERR_INVALID, "ed_gc_copy: bad arguments");
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = gc_drain(a)) return rc;
  if (a->n == 0) return ED_OK;
  HIP_TRY(hipMemcpy(gc, a->d_sums.get(), (size_t)a->n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(atgc, a->d_sums.get() + a->n, (size_t)a->n * 4, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_gc_copy")

ED_EXPORT int ed_gc_kernel_ms(ed_gc* a, double* ms)
try {
  if (!a || !ms) return ed_fail(ED_ERR_INVALID, "ed_gc_kernel_ms: NULL argument");
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = gc_drain(a)) return rc;
  *ms = a->kernel_ms;
  return ED_OK;
}
ED_CATCH("ed_gc_kernel_ms")
