// edinflate.inc -- BGZF blocks inflated and CRC-checked on the device (included at the end of edcore.hip).  DESIGN 4.25.
//
// k_bgzf_inflate: one wavefront per BGZF block.  The decoder is ed_inflate.hpp's inflate_stream, the text the host checker
// (tools/inflate_check.cpp) runs with one thread, instantiated here with a 64-lane executor: the symbol loop is serial and the same in every lane
// (the compressed bytes are read by all lanes at one address); the lanes share out the table building (a code length each), the copies of stored
// blocks and of LZ77 matches, and the CRC-32 (a slice each, shifted to its place and XOR-ed together).  Literals are collected a lane each and
// stored 64 at a time.  ISIZE is in every block's trailer, so the host knows each block's place in the inflated stream before anything is decoded
// and the blocks of a batch inflate into ONE contiguous buffer.
//
// Where the window lives: in GLOBAL memory -- the block's own slot of the output buffer, no copy in LDS.  A match reads bytes that other lanes of
// the same wavefront stored a few instructions earlier.  That is correct because (1) one wavefront's vector memory instructions are issued in
// program order to one vector L1, which serves a load behind the stores that precede it, so a load sees every earlier store of its own wavefront
// (the AMDGPU memory model needs no cache action and no wait for wavefront-scope synchronisation for that reason), and (2) the compiler is kept from
// moving the load above those stores by a wavefront-scope acquire-release fence (InfWavePrim::sync) between every store and a dependent load -- before
// each match copy, before the CRC pass, around the table building.  No other wavefront ever touches the slot.  LDS then holds only the decode
// tables (edinf::Tables, 3.9 KiB a wavefront): a 64 KiB window in LDS would let two blocks decode on a CU instead of the 16 the kernel's registers allow.
//
// Termination and bounds are the header's: every loop consumes an input bit or an output byte or leaves with a status; every store is checked
// against the block's ISIZE slot and every input read goes through the bit reader, so a corrupt block costs its own length in work, gets a status
// (a plain vector store to status[block]) and leaves its neighbours' bytes and statuses alone.
//
// The records, without a serial walk of the file (k_bam_scan_blocks, k_bam_scan_chain, k_bam_gather).  The chain off -> off + 4 + block_size is
// serial over the stream, so it is walked by guess and proof.  (1) k_bam_scan_blocks, a LANE per BGZF block (the walk is one dependent 4-byte load
// after the other: a wavefront would have one useful lane, so a lane takes a block and a wavefront 64 of them), walks from the guess that the
// block starts on a record boundary -- true for every block htslib writes -- and notes the records that START in the block, where the first
// record beyond it begins (the exit), and whether it met a bad block_size word (ed_bamscan.hpp's rule) or the end of the batch.  (2)
// k_bam_scan_chain, one lane, goes over the blocks in order: block 0's entry is the caller's (the first record after the header, or the carry
// of the batch before), block b + 1's entry is block b's exit; where the guess was the true entry its result stands, where not the block is
// walked again from its true entry -- exact for any file by induction, and a serial pass for a file whose records straddle every block.  It also
// sums the counts (the blocks' places in the record arrays).  (3) k_bam_gather, a lane per block again, walks each block from its true entry
// and writes refID, pos, tlen, flag | mapq << 16 in stream order.  Every read is checked against the end of the batch's stream; every walk
// advances by at least 36 bytes a step.  A record cut by the end of the batch is copied, device to device, in front of the next batch's stream.

namespace {

constexpr int kInfWaves = 4;                       // wavefronts = BGZF blocks of a workgroup
constexpr int kInfBlock = kInfWaves * 64;
constexpr int kInfGuard = 4;                       // guard words on either side of a batch's status array
constexpr int32_t kInfGuardWord = (int32_t)0xa5a5a5a5;

struct InfJob { int64_t out_off; uint32_t in_off, in_len, isize, pad; };

struct InfWavePrim {           // what a wavefront gives edinf::Lanes, the 64-lane executor of edinf::inflate_stream (ed_inflate.hpp)
  static constexpr int kLanes = 64;
  __device__ void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
  __device__ uint32_t xor_all(uint32_t v) const
  {
    for (int d = 32; d; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
  }
};
using InfWave = edinf::Lanes<InfWavePrim>;

static_assert(kInfBlock == 256, "k_bgzf_inflate fills the CRC table an entry a thread");

__global__ void __launch_bounds__(kInfBlock)
k_bgzf_inflate(const uint8_t* __restrict__ in, const InfJob* __restrict__ jobs, int32_t n_blocks, uint8_t* out /* the first slot */,
               int32_t* __restrict__ status)
{
  __shared__ edinf::Tables tabs[kInfWaves];
  __shared__ uint32_t crc_tab[256];
  crc_tab[threadIdx.x] = edinf::crc32_table_entry(threadIdx.x);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t b = (int64_t)blockIdx.x * kInfWaves + wv;
  if (b >= n_blocks) return;
  const InfJob j = jobs[b];
  const uint8_t* blk = in + j.in_off;
  edinf::BlockInfo bi;
  int st = edinf::block_info(blk, j.in_len, &bi);
  if (st == edinf::OK && bi.isize != j.isize) st = edinf::SIZE_MISMATCH;      // (the host read the same bytes: it cannot differ)
  if (st == edinf::OK) {
    InfWave w{out + j.out_off, 0u, j.isize, crc_tab, (int)(threadIdx.x & 63), 0u, 0u, InfWavePrim{}};
    edinf::Report rep{0, 0};
    st = edinf::inflate_stream(w, tabs[wv], blk + bi.data_off, bi.data_len, bi.crc, rep);
  }
  if ((threadIdx.x & 63) == 0) status[kInfGuard + b] = st;
}


// ---------------------------------------------------------------------------------------------- the record scan
constexpr int kScanBlock = 256;                    // threads = BGZF blocks of a workgroup of k_bam_scan_blocks and k_bam_gather

struct ScanWalk { int64_t n, exit, bad_off; int32_t flag, bad_value; };       // flag: 0 reached the block's end, 1 bad block_size, 2 cut by the batch's end
struct ScanResult {                                // what the host reads back of a batch
  int64_t n_records, consumed, excess, bad_off, total;     // consumed: the first byte not delivered; excess: the entry lies that far beyond the batch
  int32_t flag, bad_value;
};

// the records that start in [entry, end) of a stream of `total` bytes: a record counts when it lies wholly inside the stream
__device__ __forceinline__ ScanWalk scan_walk(const uint8_t* __restrict__ st, int64_t entry, int64_t end, int64_t total)
{
  ScanWalk w{0, entry, 0, 0, 0};
  int64_t off = entry;
  while (off < end) {
    if (total - off < 4) { w.flag = 2; break; }
    const int32_t bs = (int32_t)edinf::le32(st + off);
    if (bs < edbam::kFixed || bs > edbam::kMaxBlock) { w.flag = 1; w.bad_off = off; w.bad_value = bs; break; }
    if (total - off - 4 < (int64_t)bs) { w.flag = 2; break; }
    off += 4 + (int64_t)bs;
    ++w.n;
  }
  w.exit = off;
  return w;
}

// where block b's bytes begin and end in the stream (block 0 also holds the carry in front of the first slot)
__device__ __forceinline__ void scan_span(const InfJob* __restrict__ jobs, int32_t b, int64_t base, int64_t* s, int64_t* e)
{
  *s = b == 0 ? 0 : base + jobs[b].out_off;
  *e = base + jobs[b].out_off + (int64_t)jobs[b].isize;
}

__global__ void __launch_bounds__(kScanBlock)
k_bam_scan_blocks(const uint8_t* __restrict__ st, const InfJob* __restrict__ jobs, int32_t n_blocks, int64_t base, int64_t total, int64_t entry0,
                  ScanWalk* __restrict__ guess)
{
  const int32_t b = (int32_t)(blockIdx.x * kScanBlock + threadIdx.x);
  if (b >= n_blocks) return;
  int64_t s, e;
  scan_span(jobs, b, base, &s, &e);
  if (b == 0) s = entry0;
  guess[b] = scan_walk(st, s, e, total);
}

__global__ void __launch_bounds__(64)
k_bam_scan_chain(const uint8_t* __restrict__ st, const InfJob* __restrict__ jobs, int32_t n_blocks, int64_t base, int64_t total, int64_t entry0,
                 const ScanWalk* __restrict__ guess, int64_t* __restrict__ entry_of, int64_t* __restrict__ count_of, int64_t* __restrict__ first_of,
                 ScanResult* __restrict__ res)
{
  if (threadIdx.x != 0) return;
  int64_t entry = entry0, n = 0;
  ScanResult r{0, 0, 0, 0, total, 0, 0};
  for (int32_t b = 0; b < n_blocks; ++b) {
    int64_t s, e;
    scan_span(jobs, b, base, &s, &e);
    if (b == 0) s = entry0;
    entry_of[b] = entry; first_of[b] = n; count_of[b] = 0;
    if (r.flag || entry >= e) continue;
    const ScanWalk w = entry == s ? guess[b] : scan_walk(st, entry, e, total);
    count_of[b] = w.n;
    n += w.n;
    entry = w.exit;
    if (w.flag) { r.flag = w.flag; r.bad_off = w.bad_off; r.bad_value = w.bad_value; }
  }
  r.n_records = n;
  r.consumed = entry < total ? entry : total;
  r.excess = entry > total ? entry - total : 0;
  *res = r;
}

__global__ void __launch_bounds__(kScanBlock)
k_bam_gather(const uint8_t* __restrict__ st, int32_t n_blocks, const int64_t* __restrict__ entry_of, const int64_t* __restrict__ count_of,
             const int64_t* __restrict__ first_of, int64_t cap, int32_t* __restrict__ refid, int32_t* __restrict__ pos, int32_t* __restrict__ tlen,
             uint32_t* __restrict__ flag_mapq)
{
  const int32_t b = (int32_t)(blockIdx.x * kScanBlock + threadIdx.x);
  if (b >= n_blocks) return;
  int64_t off = entry_of[b], k = first_of[b];
  for (int64_t i = 0; i < count_of[b] && k < cap; ++i, ++k) {        // (the chain counted only records that lie wholly inside the stream)
    const uint8_t* r = st + off + 4;
    refid[k] = (int32_t)edinf::le32(r);
    pos[k] = (int32_t)edinf::le32(r + 4);
    tlen[k] = (int32_t)edinf::le32(r + 28);
    flag_mapq[k] = edinf::le16(r + 14) | ((uint32_t)r[9] << 16);
    off += 4 + (int64_t)(int32_t)edinf::le32(st + off);
  }
}

struct InfSet {                // one batch in flight
  PinBuf<char> pin;            // the blocks' bytes, then their jobs
  DevBuf<char> dev;            // the same on the device
  DevBuf<uint8_t> d_out;       // the inflated stream (with `gap` guard bytes before, between and after the slots when the object has a gap)
  DevBuf<int32_t> d_status;    // kInfGuard guard words, a status a block, kInfGuard guard words
  PinBuf<int32_t> h_status;
  DevBuf<char> d_scan;         // ScanWalk [n] + entry, count, first (int64 [n] each) + ScanResult
  PinBuf<ScanResult> h_res;
  DevBuf<char> d_rec;          // refid, pos, tlen, flag_mapq: [cap] each
  Event up, k0, k1, k2, k3, done;
  int64_t n_blocks = 0, n_out = 0, first_block = 0, first_byte = 0;
  int64_t base = 0, rec_cap = 0, rec_arr = 0, abs0 = 0;      // bytes of carry in front; records the arrays hold; bytes of one; the stream's place in the file's
  bool scanned = false;
  std::vector<int64_t> block_byte;   // where each block begins in the file
  bool busy = false;           // enqueued and not waited for
};

}  // namespace

struct ed_bamdev {
  int device = 0;
  int64_t batch_bytes = 0;
  int32_t gap = 0;
  int64_t n_push = 0, blocks_seen = 0, bytes_seen = 0;
  int last = -1;               // the set of the last completed batch, or -1
  int64_t first_record = -1;   // ed_bamdev_begin's: < 0 = inflate only
  int64_t entry = 0, carry = 0, carry_from = 0, abs0 = 0, records_seen = 0;      // the next batch's entry, its carry (bytes, and where they lie in the last set's stream)
  double inflate_ms = 0.0, scan_ms = 0.0, gather_ms = 0.0;
  InfSet set[2];
  Stream copy, stream;         // (declared last: they go first, after ed_bamdev_destroy has waited for them)
};

static size_t inf_up(size_t b) { return (b + 255) & ~(size_t)255; }

// waits for the batch of set k, adds its kernel's time, and looks at its statuses: ED_ERR_INVALID naming the first block that failed
static int inf_wait(ed_bamdev* a, int k)
{
  InfSet& s = a->set[k];
  if (!s.busy) return ED_OK;
  HIP_TRY(hipEventSynchronize(s.done));
  s.busy = false;
  a->last = k;
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
  a->inflate_ms += (double)ms;
  if (s.scanned) {
    HIP_TRY(hipEventElapsedTime(&ms, s.k1, s.k2));
    a->scan_ms += (double)ms;
    HIP_TRY(hipEventElapsedTime(&ms, s.k2, s.k3));
    a->gather_ms += (double)ms;
  }
  const int32_t* st = s.h_status.get();
  for (int g = 0; g < kInfGuard; ++g)
    if (st[g] != kInfGuardWord || st[kInfGuard + s.n_blocks + g] != kInfGuardWord)
      return ed_fail(ED_ERR_STATE, "ed_bamdev: a guard word of the status array was overwritten");
  for (int64_t i = 0; i < s.n_blocks; ++i)
    if (st[kInfGuard + i] != edinf::OK)
      return ed_fail(ED_ERR_INVALID, "corrupt BGZF block: block %lld of the file, at byte %lld, does not inflate: %s", (long long)(s.first_block + i),
                     (long long)s.block_byte[(size_t)i], edinf::status_name(st[kInfGuard + i]));
  if (s.scanned) {
    const ScanResult& r = *s.h_res.get();
    a->carry = r.total - r.consumed; a->carry_from = r.consumed; a->entry = r.excess;
    a->abs0 = s.abs0 + r.consumed;
    const int64_t before = a->records_seen;
    a->records_seen += r.n_records;
    if (r.flag == 1)
      return ed_fail(ED_ERR_INVALID, "ed_bamdev: record %lld at byte %lld has block_size %d (32 .. %d wanted): not a BAM record stream, or a corrupt one",
                     (long long)(before + r.n_records), (long long)(s.abs0 + r.bad_off - a->first_record), r.bad_value, edbam::kMaxBlock);
  }
  return ED_OK;
}

ED_EXPORT void ed_bamdev_destroy(ed_bamdev* a)
{
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->copy) (void)hipStreamSynchronize(a->copy);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  delete a;
}

ED_EXPORT int ed_bamdev_create(ed_bamdev** out, int device, int64_t batch_bytes)
try {
  if (!out || batch_bytes < 1 || batch_bytes > ((int64_t)1 << 30)) return ed_fail(ED_ERR_INVALID, "ed_bamdev_create: bad arguments (1 <= batch_bytes <= 2^30)");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(device));
  ed_bamdev* a = new (std::nothrow) ed_bamdev;
  if (!a) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  struct Guard { ed_bamdev* a; ~Guard() { if (a) ed_bamdev_destroy(a); } } guard{a};
  a->device = device; a->batch_bytes = batch_bytes;
  for (Stream* s : {&a->stream, &a->copy}) {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s->reset(st);
  }
  for (InfSet& s : a->set) {
    HIP_TRY(s.up.create(hipEventDisableTiming));
    HIP_TRY(s.k0.create());
    HIP_TRY(s.k1.create());
    HIP_TRY(s.k2.create());
    HIP_TRY(s.k3.create());
    HIP_TRY(s.done.create(hipEventDisableTiming));
    if (s.h_res.alloc(sizeof(ScanResult)) != hipSuccess) return ed_fail(ED_ERR_NOMEM, "ed_bamdev_create: pinned allocation failed");
  }
  guard.a = nullptr;
  *out = a;
  return ED_OK;
}
ED_CATCH("ed_bamdev_create")

// a new file: nothing in flight, block, byte and record counts from zero.  first_record_offset: where the first record begins in the
// inflated stream (after the BAM header), or < 0 to inflate only
ED_EXPORT int ed_bamdev_begin(ed_bamdev* a, int64_t first_record_offset)
try {
  if (!a) return ed_fail(ED_ERR_INVALID, "ed_bamdev_begin: NULL object");
  HIP_TRY(hipSetDevice(a->device));
  HIP_TRY(hipStreamSynchronize(a->copy));
  HIP_TRY(hipStreamSynchronize(a->stream));
  for (InfSet& s : a->set) { s.busy = false; s.scanned = false; }
  a->gap = 0; a->n_push = 0; a->blocks_seen = 0; a->bytes_seen = 0; a->last = -1;
  a->first_record = first_record_offset; a->entry = first_record_offset < 0 ? 0 : first_record_offset;
  a->carry = 0; a->carry_from = 0; a->abs0 = 0; a->records_seen = 0;
  return ED_OK;
}
ED_CATCH("ed_bamdev_begin")

// for tests, after ed_bamdev_begin: `gap` guard bytes before, between and after the blocks' output slots (the stream is then not contiguous: no scan)
ED_EXPORT int ed_bamdev_set_guard_gap(ed_bamdev* a, int32_t gap)
try {
  if (!a || gap < 0 || gap > 4096) return ed_fail(ED_ERR_INVALID, "ed_bamdev_set_guard_gap: bad arguments");
  if (a->n_push) return ed_fail(ED_ERR_STATE, "ed_bamdev_set_guard_gap: after ed_bamdev_begin and before the first push");
  a->gap = gap;
  if (gap > 0) a->first_record = -1;
  return ED_OK;
}
ED_CATCH("ed_bamdev_set_guard_gap")

ED_EXPORT int ed_bamdev_push(ed_bamdev* a, const uint8_t* buf, int64_t n_bytes, int64_t* bytes_consumed, int64_t* n_records)
try {
  if (!a || n_bytes < 0 || !bytes_consumed || !n_records || (n_bytes > 0 && !buf)) return ed_fail(ED_ERR_INVALID, "ed_bamdev_push: bad arguments");
  *bytes_consumed = 0; *n_records = 0;
  HIP_TRY(hipSetDevice(a->device));
  const int k = (int)(a->n_push & 1);
  InfSet& s = a->set[k];
  if (int rc = inf_wait(a, k)) return rc;                 // (two batches back: long complete unless the caller ignored an error)
  // the whole blocks at the front of buf, up to batch_bytes of them (one at least)
  std::vector<InfJob> jobs;
  s.block_byte.clear();
  int64_t off = 0, out_off = a->gap;                      // (slots are placed relative to the first one: the carry in front is known later)
  while (off < n_bytes) {
    const int32_t size = edinf::bgzf_block_size(buf + off, n_bytes - off);
    if (size < 0) return ed_fail(ED_ERR_INVALID, "not a BGZF file: no BGZF block header at byte %lld", (long long)(a->bytes_seen + off));
    if (size == 0 || size > n_bytes - off || (!jobs.empty() && off + size > a->batch_bytes)) break;
    const uint32_t isize = edinf::le32(buf + off + size - 4);
    if (isize > edinf::kMaxInflated)
      return ed_fail(ED_ERR_INVALID, "corrupt BGZF block: block %lld of the file, at byte %lld, names an inflated size of %u (at most 65536)",
                     (long long)(a->blocks_seen + (int64_t)jobs.size()), (long long)(a->bytes_seen + off), isize);
    jobs.push_back(InfJob{out_off, (uint32_t)off, (uint32_t)size, isize, 0u});
    s.block_byte.push_back(a->bytes_seen + off);
    out_off += (int64_t)isize + a->gap;
    off += size;
  }
  const int64_t nb = (int64_t)jobs.size();
  const size_t in_bytes = inf_up((size_t)off), need = in_bytes + inf_up((size_t)nb * sizeof(InfJob));
  const size_t st_bytes = (size_t)(nb + 2 * kInfGuard) * 4;
  if (nb > 0) {
    if (s.pin.reserve(need) != hipSuccess || s.dev.reserve(need) != hipSuccess
        || s.d_status.reserve(st_bytes) != hipSuccess || s.h_status.reserve(st_bytes) != hipSuccess)
      return ed_fail(ED_ERR_NOMEM, "ed_bamdev_push: allocation of %zu bytes failed", 2 * need + (size_t)out_off + 2 * st_bytes);
    std::memcpy(s.pin.get(), buf, (size_t)off);
    std::memcpy(s.pin.get() + in_bytes, jobs.data(), (size_t)nb * sizeof(InfJob));
    // the upload goes on the copy stream, under the kernel of the batch before
    HIP_TRY(hipMemcpyAsync(s.dev, s.pin, need, hipMemcpyHostToDevice, a->copy));
    HIP_TRY(hipEventRecord(s.up, a->copy));
  }
  const bool waited = a->set[k ^ 1].busy;
  if (int rc = inf_wait(a, k ^ 1)) return rc;             // the batch before: its statuses and its scan decide whether the file goes on
  if (waited && a->set[a->last].scanned) *n_records = a->set[a->last].h_res.get()->n_records;
  if (nb == 0) return ED_OK;
  const bool scan = a->first_record >= 0;
  const int64_t base = scan ? a->carry : 0, total = base + out_off;
  if (s.d_out.reserve((size_t)std::max<int64_t>(total, 1)) != hipSuccess)
    return ed_fail(ED_ERR_NOMEM, "ed_bamdev_push: device allocation of %lld bytes failed", (long long)total);
  const size_t walk_b = inf_up((size_t)nb * sizeof(ScanWalk)), arr_b = inf_up((size_t)nb * 8);
  const int64_t cap = total / 36 + 1;
  const size_t rec_arr = inf_up((size_t)cap * 4);
  if (scan && (s.d_scan.reserve(walk_b + 3 * arr_b + sizeof(ScanResult)) != hipSuccess || s.d_rec.reserve(4 * rec_arr) != hipSuccess))
    return ed_fail(ED_ERR_NOMEM, "ed_bamdev_push: device allocation of %zu bytes failed", walk_b + 3 * arr_b + 4 * rec_arr);
  HIP_TRY(hipStreamWaitEvent(a->stream, s.up, 0));
  HIP_TRY(hipMemsetAsync(s.d_status, 0xa5, st_bytes, a->stream));
  if (a->gap > 0) HIP_TRY(hipMemsetAsync(s.d_out, 0xa5, (size_t)out_off, a->stream));
  if (base > 0)                                             // the record the batch before ended in, in front of this batch's blocks
    HIP_TRY(hipMemcpyAsync(s.d_out.get(), a->set[k ^ 1].d_out.get() + a->carry_from, (size_t)base, hipMemcpyDeviceToDevice, a->stream));
  const InfJob* d_jobs = (const InfJob*)(s.dev.get() + in_bytes);
  HIP_TRY(hipEventRecord(s.k0, a->stream));
  hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned int)((nb + kInfWaves - 1) / kInfWaves)), dim3(kInfBlock), 0, a->stream,
                     (const uint8_t*)s.dev.get(), d_jobs, (int32_t)nb, s.d_out.get() + base, s.d_status.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.k1, a->stream));
  if (scan) {
    char* d = s.d_scan.get();
    ScanWalk* guess = (ScanWalk*)d;
    int64_t* entry_of = (int64_t*)(d + walk_b);
    int64_t* count_of = (int64_t*)(d + walk_b + arr_b);
    int64_t* first_of = (int64_t*)(d + walk_b + 2 * arr_b);
    ScanResult* res = (ScanResult*)(d + walk_b + 3 * arr_b);
    const unsigned int grid = (unsigned int)((nb + kScanBlock - 1) / kScanBlock);
    hipLaunchKernelGGL(k_bam_scan_blocks, dim3(grid), dim3(kScanBlock), 0, a->stream, (const uint8_t*)s.d_out.get(), d_jobs, (int32_t)nb, base, total,
                       a->entry, guess);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan_chain, dim3(1), dim3(64), 0, a->stream, (const uint8_t*)s.d_out.get(), d_jobs, (int32_t)nb, base, total, a->entry,
                       (const ScanWalk*)guess, entry_of, count_of, first_of, res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.k2, a->stream));
    char* rec = s.d_rec.get();
    hipLaunchKernelGGL(k_bam_gather, dim3(grid), dim3(kScanBlock), 0, a->stream, (const uint8_t*)s.d_out.get(), (int32_t)nb, (const int64_t*)entry_of,
                       (const int64_t*)count_of, (const int64_t*)first_of, cap, (int32_t*)rec, (int32_t*)(rec + rec_arr), (int32_t*)(rec + 2 * rec_arr),
                       (uint32_t*)(rec + 3 * rec_arr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.k3, a->stream));
    HIP_TRY(hipMemcpyAsync(s.h_res.get(), res, sizeof(ScanResult), hipMemcpyDeviceToHost, a->stream));
  }
  HIP_TRY(hipMemcpyAsync(s.h_status, s.d_status, st_bytes, hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipEventRecord(s.done, a->stream));
  s.busy = true; s.scanned = scan;
  s.n_blocks = nb; s.n_out = total; s.first_block = a->blocks_seen; s.first_byte = a->bytes_seen;
  s.base = base; s.rec_cap = cap; s.rec_arr = (int64_t)rec_arr; s.abs0 = a->abs0;
  a->blocks_seen += nb; a->bytes_seen += off;
  ++a->n_push;
  *bytes_consumed = off;
  return ED_OK;
}
ED_CATCH("ed_bamdev_push")

ED_EXPORT int ed_bamdev_end(ed_bamdev* a)
try {
  if (!a) return ed_fail(ED_ERR_INVALID, "ed_bamdev_end: NULL object");
  HIP_TRY(hipSetDevice(a->device));
  const int k = (int)(a->n_push & 1);                       // the older of the two first
  if (int rc = inf_wait(a, k)) return rc;
  if (int rc = inf_wait(a, k ^ 1)) return rc;
  if (a->first_record >= 0 && (a->carry > 0 || a->entry > 0)) {
    const int64_t left = a->carry;
    const bool header = a->entry > 0;
    a->carry = 0; a->entry = 0;
    if (header) return ed_fail(ED_ERR_INVALID, "truncated BAM: the stream ends before the first record");
    return ed_fail(ED_ERR_INVALID, "truncated BAM: %lld bytes of an incomplete record at the end of the stream", (long long)left);
  }
  return ED_OK;
}
ED_CATCH("ed_bamdev_end")

// the four DEVICE arrays (refID, pos, tlen: int32; flag | mapq << 16: uint32) of the last batch waited for, *n records each, in stream order; they
// stand until the second push after the one that returned them
ED_EXPORT int ed_bamdev_records(ed_bamdev* a, int64_t* n, void* d_ptrs[4])
try {
  if (!a || !n || !d_ptrs) return ed_fail(ED_ERR_INVALID, "ed_bamdev_records: NULL argument");
  *n = 0;
  for (int k = 0; k < 4; ++k) d_ptrs[k] = nullptr;
  if (a->last < 0 || !a->set[a->last].scanned) return ED_OK;
  const InfSet& s = a->set[a->last];
  *n = s.h_res.get()->n_records;
  for (int k = 0; k < 4; ++k) d_ptrs[k] = s.d_rec.get() + (size_t)k * (size_t)s.rec_arr;
  return ED_OK;
}
ED_CATCH("ed_bamdev_records")

ED_EXPORT int ed_bamdev_block_status(ed_bamdev* a, int64_t cap, int32_t* status, int64_t* n_blocks)
try {
  if (!a || cap < 0 || !n_blocks || (cap > 0 && !status)) return ed_fail(ED_ERR_INVALID, "ed_bamdev_block_status: bad arguments");
  *n_blocks = a->last < 0 ? 0 : a->set[a->last].n_blocks;
  if (a->last >= 0) std::memcpy(status, a->set[a->last].h_status.get() + kInfGuard, (size_t)std::min(cap, *n_blocks) * 4);
  return ED_OK;
}
ED_CATCH("ed_bamdev_block_status")

ED_EXPORT int ed_bamdev_copy_inflated(ed_bamdev* a, uint8_t* out, int64_t cap, int64_t* n)
try {
  if (!a || cap < 0 || !n || (cap > 0 && !out)) return ed_fail(ED_ERR_INVALID, "ed_bamdev_copy_inflated: bad arguments");
  HIP_TRY(hipSetDevice(a->device));
  *n = a->last < 0 ? 0 : a->set[a->last].n_out;
  if (cap < *n) return ed_fail(ED_ERR_INVALID, "ed_bamdev_copy_inflated: %lld bytes, room for %lld", (long long)*n, (long long)cap);
  if (*n > 0) HIP_TRY(hipMemcpy(out, a->set[a->last].d_out.get(), (size_t)*n, hipMemcpyDeviceToHost));
  return ED_OK;
}
ED_CATCH("ed_bamdev_copy_inflated")

ED_EXPORT int ed_bamdev_kernel_ms(ed_bamdev* a, double out[3])
try {
  if (!a || !out) return ed_fail(ED_ERR_INVALID, "ed_bamdev_kernel_ms: NULL argument");
  out[0] = a->inflate_ms; out[1] = a->scan_ms; out[2] = a->gather_ms;
  return ED_OK;
}
ED_CATCH("ed_bamdev_kernel_ms")

// out = {BGZF blocks of a workgroup of k_bgzf_inflate, its threads, bytes of LDS tables a block takes, BGZF blocks of a workgroup of the scan and the gather}
ED_EXPORT int ed_bamdev_geometry(int32_t out[4])
try {
  if (!out) return ed_fail(ED_ERR_INVALID, "ed_bamdev_geometry: NULL output");
  out[0] = kInfWaves; out[1] = kInfBlock; out[2] = (int32_t)sizeof(edinf::Tables); out[3] = kScanBlock;
  return ED_OK;
}
ED_CATCH("ed_bamdev_geometry")
