// edcohort.inc -- the cohort pipeline: slabs of a cohort through batch objects in rotation, on the library's OWN streams,
// and the ingest of count matrices from host memory (pinned double buffer, copy stream, 16-bit wire format, the
// transposition from R's column-major layout).  Included by edcore.hip.
//
// What it replaces in the reference: the user's loop over samples (vignette/vignette.Rnw:390-431) -- one
// new('ExomeDepth') (R/class_definition.R:82-191: aod::betabin, then .Call get_loglike_matrix) and one CallCNVs()
// (R/class_definition.R:311-419: one .Call C_hmm per chromosome) per sample -- by one submission per SLAB of samples.
//
// Schedule of a stream of slabs (DESIGN.md 4.10), built from stream order alone -- no host timing, no environment:
//   main stream   emissions of slab t, t+1, ... back to back; each launch is cut in two with an event in between
//   fit stream    dispersion fit of slab t+1: waits for the event INSIDE slab t's emission launch, so its CU-exclusive
//                 workgroups (147 KB of LDS) are served by reservation while those emissions drain, and for the emission
//                 kernels of slab t+1-n (they read the per-sample constants made from the slot's previous (phi, expected))
//   batch streams Viterbi chains, trace-back and call table of slab t start when its emissions are through and ride
//                 underneath the start of slab t+1's emissions (ed_batch_set_async_tail)
// Every stream of the pipeline can be given a hardware queue of its own (ed_stream_create), so which of them run side by
// side does not depend on GPU_MAX_HW_QUEUES or on how many streams the process used before.

namespace {

// ---- layout kernels ----------------------------------------------------------------------------
// R hands matrices over column-major: an E x n integer matrix is n contiguous columns of E exons (sample-major).  The
// pipeline wants sample-minor rows [E][n] (a wave reads 64 consecutive samples of one exon).  64 x 64 tiles through LDS;
// T = int32_t, or uint16_t for the 16-bit wire format (counts below 65536: half the PCIe bytes), widened here.
template <class T>
__global__ void __launch_bounds__(256)
k_cols_to_rows(const T* __restrict__ in /* [n][E] */, int64_t E, int64_t n, int32_t* __restrict__ out /* [E][n] */)
{
  __shared__ int32_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 64 x 4
  const int64_t e0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t s = s0 + ty + 4 * k, e = e0 + tx;
    tile[ty + 4 * k][tx] = (s < n && e < E) ? (int32_t)in[s * E + e] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t e = e0 + ty + 4 * k, s = s0 + tx;
    if (e < E && s < n) out[e * n + s] = tile[tx][ty + 4 * k];
  }
}

// 16-bit wire format, layout unchanged
__global__ void __launch_bounds__(256) k_widen_u16(const uint16_t* __restrict__ in, int64_t count, int32_t* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) out[i] = (int32_t)in[i];
}

// [E][n] (sample-minor) -> [n][E]: the E x n matrix R would hold (the Viterbi path as raw, an aggregate reference as integer)
template <class T>
__global__ void __launch_bounds__(256)
k_rows_to_cols(const T* __restrict__ in /* [E][n] */, int64_t E, int64_t n, T* __restrict__ out /* [n][E] */)
{
  __shared__ T tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t e0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t e = e0 + ty + 4 * k, s = s0 + tx;
    tile[ty + 4 * k][tx] = (e < E && s < n) ? in[e * n + s] : (T)0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t s = s0 + ty + 4 * k, e = e0 + tx;
    if (s < n && e < E) out[s * E + e] = tile[tx][ty + 4 * k];
  }
}

}  // namespace

// ---- pinned host memory ------------------------------------------------------------------------
ED_EXPORT int ed_host_alloc(void** hptr, size_t bytes)
try {
  if (!hptr) return ed_fail(ED_ERR_INVALID, "ed_host_alloc: NULL output pointer");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
  return ED_OK;
}
ED_CATCH("ed_host_alloc")
ED_EXPORT int ed_host_free(void* hptr)
try {
  if (hptr) HIP_TRY(hipHostFree(hptr));
  return ED_OK;
}
ED_CATCH("ed_host_free")

// ---- ingest ------------------------------------------------------------------------------------
// Host block -> device, through two pinned staging buffers unless the block is pinned memory already (then the DMA engine
// reads it in place).  The copy of chunk k+1 into its staging buffer (host threads) overlaps the DMA of chunk k.
// A few host threads that stay: the staging passes hand them a job per chunk (64 MB), and starting 7 - 15 threads per chunk cost a third of a
// millisecond against the 1.3 ms the chunk's copy takes -- 8 of the R-level entry's 30 ms per cohort (round 6).  run(f) calls f(t) for t = 0 .. n - 1
// (t = 0 on the calling thread) and returns when all are done.  One job at a time (the stager is used by one thread).
struct ed_stage_workers {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  std::function<void(int)> job;
  uint64_t epoch = 0;
  int pending = 0;
  bool quit = false;
  int n = 1;
  void start(int n_threads)
  {
    n = std::max(1, n_threads);
    for (int t = 1; t < n; ++t)
      th.emplace_back([this, t] {
        uint64_t seen = 0;
        for (;;) {
          std::function<void(int)> f;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv_go.wait(lk, [&] { return quit || epoch != seen; });
            if (quit) return;
            seen = epoch;
            f = job;
          }
          try { f(t); } catch (...) {}
          {
            std::lock_guard<std::mutex> lk(mu);
            if (--pending == 0) cv_done.notify_one();
          }
        }
      });
  }
  void run(const std::function<void(int)>& f, int n_use)
  {
    n_use = std::max(1, std::min(n_use, n));
    if (n_use == 1) { f(0); return; }
    {
      std::lock_guard<std::mutex> lk(mu);
      job = [&f, n_use](int t) { if (t < n_use) f(t); };
      pending = n - 1;
      ++epoch;
    }
    cv_go.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
  ~ed_stage_workers()
  {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv_go.notify_all();
    for (auto& x : th) if (x.joinable()) x.join();
  }
};

struct ed_stager {
  int device = 0;
  double dbg_wait = 0, dbg_conv = 0; int64_t dbg_chunks = 0;
  ~ed_stager() { if (getenv("ED_STAGE_TIMING")) fprintf(stderr, "[stager] narrow: %lld chunks, waiting for a buffer %.1f ms, converting %.1f ms\n", (long long)dbg_chunks, dbg_wait * 1e3, dbg_conv * 1e3); }
  ed_stage_workers workers;
  size_t chunk = 0;
  PinBuf<void> pin[2];
  Event freed[2];                             // the DMA that last read pin[i] is complete
  bool used[2] = {false, false};
  int next = 0;
  int n_threads = 4;
  // running totals (ed_cohort_ingest_stats)
  double bytes = 0, seconds_host = 0;
};

static int stager_make(std::unique_ptr<ed_stager>& out, int device, size_t chunk_bytes)
{
  std::unique_ptr<ed_stager> g(new (std::nothrow) ed_stager);
  if (!g) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  g->device = device;
  g->chunk = std::max<size_t>(chunk_bytes, 1 << 20);
  // (16: a staging thread moves ~7 GB/s of pageable memory; narrowing R's int32 counts reads 4 bytes for every 2 it puts on the link, and with 8 threads
  //  the R-level entry was bound by that read -- 30 ms per 200 000 x 1024 cohort against 17 for counts that arrive 16 bits wide)
  g->n_threads = (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
  {
    // A container's CPU quota (cgroup v2 cpu.max "quota period", v1 cpu.cfs_quota_us / cpu.cfs_period_us): staging threads + the pipeline's own thread + the
    // runtime's beyond it get the whole process throttled for the rest of the scheduler period (seen on the GPU boxes of this project, quota 16 of 256 logical
    // CPUs: the same call 20.6 ms with 12 staging threads, 21.6-29.7 with 16).  Four cores are left to everything else.
    double cores = 0.0;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      double per = 0.0;
      if (std::fscanf(f, "%31s %lf", q, &per) == 2 && q[0] != 'm' && per > 0.0) cores = std::atof(q) / per;
      std::fclose(f);
    } else {
      double quota = -1.0, per = 0.0;
      if (FILE* f1 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(f1, "%lf", &quota) != 1) quota = -1.0; std::fclose(f1); }
      if (FILE* f2 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(f2, "%lf", &per) != 1) per = 0.0; std::fclose(f2); }
      if (quota > 0.0 && per > 0.0) cores = quota / per;
    }
    if (cores > 0.0) g->n_threads = std::max(2, std::min(g->n_threads, (int)cores - 4));
  }
  if (const char* ev = std::getenv("EXOMEDEPTH_AMD_STAGE_THREADS")) {              // (a knob for hosts with few cores per device, or many)
    const long v = std::strtol(ev, nullptr, 10);
    if (v >= 1 && v <= 64) g->n_threads = (int)v;
  }
  g->workers.start(g->n_threads);
  for (int i = 0; i < 2; ++i) {
    if (g->pin[i].alloc(g->chunk) != hipSuccess || g->freed[i].create(hipEventDisableTiming) != hipSuccess)
      return ed_fail(ED_ERR_NOMEM, "ingest: cannot allocate %zu bytes of pinned staging memory", chunk_bytes);
  }
  out = std::move(g);
  return ED_OK;
}

// The stream and the stager of one host-fed call.  Declared after the call's device buffers, so that it goes before them: the stream
// is waited for, then destroyed, then the stager goes.
struct HostFeed {
  std::unique_ptr<ed_stager> g;
  Stream s;
  int open(int dev)
  {
    HIP_TRY(ed_stream_create(s, false, dev));
    return stager_make(g, dev, (size_t)64 << 20);
  }
  ~HostFeed() { if (s) (void)hipStreamSynchronize(s); }
};

static bool host_block_is_pinned(const void* p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

// rows x row_bytes from `src` (rows src_pitch bytes apart) to the dense device block `dst`, ordered on `st`
static int stager_upload(ed_stager* g, const void* src, size_t rows, size_t row_bytes, size_t src_pitch, void* dst, hipStream_t st)
{
  if (rows == 0 || row_bytes == 0) return ED_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const bool dense = (src_pitch == row_bytes);
  if (host_block_is_pinned(src)) {
    if (dense) HIP_TRY(hipMemcpyAsync(dst, src, rows * row_bytes, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpy2DAsync(dst, row_bytes, src, src_pitch, row_bytes, rows, hipMemcpyHostToDevice, st));
  } else {
    // pageable memory: gather into a pinned buffer with a few host threads, DMA from there
    const size_t rows_per_chunk = dense ? 0 : std::max<size_t>(g->chunk / row_bytes, 1);
    const size_t total = rows * row_bytes;
    size_t done_rows = 0, done_bytes = 0;
    while (dense ? done_bytes < total : done_rows < rows) {
      const int i = g->next;
      g->next ^= 1;
      if (g->used[i]) HIP_TRY(hipEventSynchronize(g->freed[i]));
      size_t nbytes;
      if (dense) {
        nbytes = std::min(g->chunk, total - done_bytes);
        const char* s0 = (const char*)src + done_bytes;
        const int nt = (nbytes >= ((size_t)4 << 20)) ? g->n_threads : 1;
        char* const dstp = g->pin[i].as<char>();
        g->workers.run([=](int t) {
          const size_t a = nbytes * (size_t)t / nt, z = nbytes * (size_t)(t + 1) / nt;
          std::memcpy(dstp + a, s0 + a, z - a);
        }, nt);
      } else {
        const size_t nr = std::min(rows_per_chunk, rows - done_rows);
        nbytes = nr * row_bytes;
        const char* s0 = (const char*)src + done_rows * src_pitch;
        const int nt = (nbytes >= ((size_t)4 << 20)) ? g->n_threads : 1;
        char* const dstp = g->pin[i].as<char>();
        g->workers.run([=](int t) {
          const size_t a = nr * (size_t)t / nt, z = nr * (size_t)(t + 1) / nt;
          for (size_t r = a; r < z; ++r) std::memcpy(dstp + r * row_bytes, s0 + r * src_pitch, row_bytes);
        }, nt);
        done_rows += nr;
      }
      HIP_TRY(hipMemcpyAsync((char*)dst + done_bytes, g->pin[i], nbytes, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(g->freed[i], st));
      g->used[i] = true;
      done_bytes += nbytes;
    }
  }
  g->bytes += (double)(rows * row_bytes);
  g->seconds_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return ED_OK;
}

// `count` int32 counts from pageable host memory to a dense DEVICE uint16 block: the host threads that stage a chunk into the pinned double buffer
// narrow it while they copy (the copy has to touch every count anyway), so the link carries 2 bytes per count.  R's integers are 32 bits wide
// (reference R/class_definition.R:82-93: `test` / `reference`), read counts of exome data are not: a chunk holding a count outside 0 .. 65 535
// stops the upload with *wide = true and the caller sends the slab as int32 instead.
static int stager_upload_narrow(ed_stager* g, const int32_t* src, size_t count, uint16_t* dst, hipStream_t st, bool* wide)
{
  *wide = false;
  if (count == 0) return ED_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t per = g->chunk / 2;                       // counts per staging buffer
  for (size_t done = 0; done < count;) {
    const int i = g->next;
    g->next ^= 1;
    const auto tw0 = std::chrono::steady_clock::now();
    if (g->used[i]) HIP_TRY(hipEventSynchronize(g->freed[i]));
    const auto tw1 = std::chrono::steady_clock::now();
    g->dbg_wait += std::chrono::duration<double>(tw1 - tw0).count();
    const size_t n = std::min(per, count - done);
    const int32_t* s0 = src + done;
    uint16_t* p = g->pin[i].as<uint16_t>();
    const int nt = (n >= ((size_t)1 << 20)) ? g->n_threads : 1;
    std::vector<uint32_t> seen((size_t)nt, 0u);
    uint32_t* const seenp = seen.data();
    g->workers.run([=](int t) {
      // Four counts per 8-byte NON-TEMPORAL store: the staging buffer is written once and read by the DMA engine -- ordinary stores first READ every
      // line they are about to overwrite (0.8 GB per cohort on top of the 1.6 GB of int32 read), which is what memcpy's large-copy path avoids too.
      size_t a = n * (size_t)t / nt, z = n * (size_t)(t + 1) / nt;
      a &= ~(size_t)31; if (t + 1 < nt) z &= ~(size_t)31;            // (whole 64-byte lines of the buffer per thread; the buffers are 4 KB-aligned)
      uint32_t acc = 0;
      size_t k = a;
      for (; k + 4 <= z; k += 4) {
        const uint32_t v0 = (uint32_t)s0[k], v1 = (uint32_t)s0[k + 1], v2 = (uint32_t)s0[k + 2], v3 = (uint32_t)s0[k + 3];
        acc |= (v0 | v1) | (v2 | v3);
        const uint64_t w = (uint64_t)(v0 & 0xffffu) | ((uint64_t)(v1 & 0xffffu) << 16) | ((uint64_t)(v2 & 0xffffu) << 32) | ((uint64_t)(v3 & 0xffffu) << 48);
        __builtin_nontemporal_store(w, (uint64_t*)(p + k));
      }
      for (; k < z; ++k) { const uint32_t v = (uint32_t)s0[k]; acc |= v; p[k] = (uint16_t)v; }
      seenp[t] = acc;
    }, nt);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);               // (the weakly ordered stores are globally visible before the copy is issued)
    g->dbg_conv += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw1).count();
    g->dbg_chunks += 1;
    uint32_t acc = 0;
    for (uint32_t v : seen) acc |= v;
    if (acc > 0xffffu) {                                  // (a negative count has its high bits set)
      *wide = true;
      g->next ^= 1;                                       // the buffer was not handed to the DMA engine
      g->seconds_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return ED_OK;
    }
    HIP_TRY(hipMemcpyAsync(dst + done, p, n * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(g->freed[i], st));
    g->used[i] = true;
    done += n;
  }
  g->bytes += (double)count * 2;
  g->seconds_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return ED_OK;
}

// ---- cohort ------------------------------------------------------------------------------------
struct ed_cohort {
  ed_plan* plan = nullptr;
  int64_t slab = 0;
  int n_slots = 0;
  struct Slot {
    std::unique_ptr<ed_batch> batch; // sized for the nominal slab
    std::unique_ptr<ed_batch> odd;   // sized for a ragged slab (made when one is submitted)
    ed_batch* cur = nullptr;         // borrowed: the one of the two that holds the slot's current ticket
    DevBuf<double> d_phi, d_exp;     // [slab] (phi, expected) of the slot's ticket: fitted here, or copied from the caller's
    Event emitted;                   // main stream: the emission kernels of the slot's last run are through
    Event fitted;                    // fit stream: the slot's (phi, expected) are complete
    Event ready;                     // the slab's counts are complete on the caller's / the copy stream
    bool emitted_set = false;
    int64_t ticket = -1;
    int64_t n = 0;
    // host-fed slabs (ed_cohort_run_host / ed_cohort_submit_host): counts owned by the slot
    DevBuf<int32_t> own_test, own_ref;
    DevBuf<char> raw;                // staging for the layouts that need a device pass (2 matrices)
    DevBuf<uint8_t> path_cols;       // [n][E] copy of the path for the column-major output
    // depth-binned dispersion (option phi_bins > 1): phi.estimates [8][slab] and complete.bins [9][slab] of the slot's ticket; the
    // fit is issued without a look at its outcome, which is settled when the ticket is first waited for (cohort_bins_settle)
    DevBuf<double> d_phib, d_edges;
    bool bins_pending = false;
    const int32_t* last_test = nullptr;   // borrowed: the counts of the slot's ticket (the caller's, or own_test / own_ref)
    const int32_t* last_ref = nullptr;
    double last_mix = 1.0;
    const double* last_mix_s = nullptr;   // ... and its per-sample mixtures (ed_cohort_submit_mix), if any
    int lane = 0;
  };
  // (declared ahead of the slots, the stager and the buffers: members go in reverse order, so the streams outlive everything queued on them)
  static constexpr int kMaxLanes = 4;
  Stream mains[kMaxLanes], fits[kMaxLanes];
  Stream copy;
  std::vector<Slot> slots;
  // LANES (round 5): independent pipelines inside one cohort object.  Slot s belongs to lane s % n_lanes; a lane has its own emission ("main") and fit
  // streams and its slots' batch objects their own side / tail streams, so nothing orders the slabs of different lanes against each other.  Why: one
  // pipeline's emission stream carries emit(t), then the constants / table statistics / table build of t + 1, then emit(t + 1), strictly in turn, and
  // while that preparation runs (beside the chains of t) most CUs have nothing to do; a second pipeline's emission launch fills them.  Measured on
  // 200 000 x 1024 slabs, fit on (tools/lanes_probe.py; two PROCESSES sharing the GPU showed it first): 1 lane x 2 slots 4.04 ms per slab, 2 x 2 3.70,
  // 3 x 2 3.63; 2 x 1 3.8-3.96.  Option "lanes" (before the first submission): 1 (default) = the one pipeline the object was before; 2 .. 4 = that many
  // (a divisor of slabs_in_flight); 0 = slabs_in_flight / 2 lanes of two slots when slabs_in_flight is 4, 6 or 8.  Opt-in, because it pays where a slab
  // fills the chip and is fitted on the device (the bench's headline: 3.9 against 4.2 ms); measured WORSE for 64-sample slabs with given parameters
  // (six slabs in flight as three lanes: 1.56 ms per slab against 0.66 as one lane -- that pipeline lives on its one fit stream running ahead) and
  // for host-fed slabs (link-bound: 21.4 against 16.1 ms).
  int n_lanes = 1, lanes_opt = 1;
  bool pipelined() const { return n_slots / n_lanes >= 2; }     // a lane with two or more slots overlaps the stages of its consecutive slabs
  int64_t next_ticket = 0;
  bool started = false;
  bool timing = false;
  Event epoch;                       // option timing: recorded (and waited for) when the option is set; the emission launches' intervals are relative to it
  std::vector<float> emit_iv;        // (start_ms, end_ms) of the emission stage of every timed run, in the order the runs were folded
  // options
  double split_frac = 0.30;
  bool split_set = false;            // the caller chose `split` (otherwise emit mode 2 runs without a cut)
  bool own_queues = true;
  int bins_pieces = 10;              // phi_bins > 1, pipelined: launches per slab of the emission kernel (boundaries at which the next
                                     // slab's fit kernels get their CUs)
  int phi_bins = 1;                  // > 1: the depth-binned dispersion model (R/class_definition.R:120-147) for every slab
  std::vector<double> h_phib, h_edges;   // ed_cohort_run_host in that mode: [phi_bins][S_total], [(phi_bins + 1)][S_total]
  int fit_mode = 0;                  // 0: maximum likelihood (Newton on histograms); 1: aod::betabin's Nelder-Mead procedure
  int emit_mode = 0;                 // 0: strict emissions; 1: log-gamma difference tables (edtab.inc); 2: ... sample-major
  int counts_layout = 0;             // 0: device count matrices [E][n]; 1: [n][E] (sample-major = R's column-major E x n matrix; emit mode 2)
  int counts_bits = 32;              // 16: the DEVICE count matrices of ed_cohort_submit are uint16 (counts_layout 1 + emit mode 2 only; host-fed slabs choose per slab)
  int emit_tails = 1;                // emit mode 2: tail samples on (ed_batch_set_emit_tails)
  bool host_narrow = true;           // host-fed slabs of a sample-major table cohort are kept 16 bits wide on the device whenever their counts fit (option host_narrow)
  int64_t n_wide_slabs = 0;          // host-fed int32 slabs that held a count beyond 65 535 and went up as int32 (ed_cohort_ingest_stats)
  int viterbi_overlap = 0;
  bool tables_early = false;         // per-sample constants and tables of a slab right behind its fit, on the fit stream (measured:
                                     // the boundary between two emission launches shrinks by 0.3 ms and the launch that hosts them grows
                                     // by as much -- 10.26-10.41 against 10.27-10.35 ms per step -- so the default keeps them at the boundary)
  std::unique_ptr<ed_stager> stager;
  DevBuf<double> d_par;              // ed_cohort_run_host with given parameters: (phi[S_total], expected[S_total]) on the device; grow-only
  DevBuf<double> d_mixv;             // ed_cohort_run_host_mix: the per-sample mixtures [S_total] on the device; grow-only
  // results of ed_cohort_run_host
  std::vector<ed_call> calls;
  std::vector<ed_call_info> info;
  int64_t n_unconverged = 0;
  int64_t n_gsl_errors = 0;
  int64_t tab_stats[4] = {0, 0, 0, 0};   // ed_batch_table_stats summed over the slabs of the last ed_cohort_run_host
};

ED_EXPORT int ed_cohort_create(ed_cohort** cohort, ed_plan* plan, int64_t slab_samples, int slabs_in_flight)
try {
  if (!cohort || !plan || slab_samples <= 0 || slabs_in_flight < 1 || slabs_in_flight > 8)
    return ed_fail(ED_ERR_INVALID, "ed_cohort_create: bad arguments (1 <= slabs_in_flight <= 8)");
  if (int rc = require_device()) return rc;
  HIP_TRY(hipSetDevice(plan->device));
  ed_cohort* c = new (std::nothrow) ed_cohort;
  if (!c) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  c->plan = plan; c->slab = slab_samples; c->n_slots = slabs_in_flight;
  c->slots.resize((size_t)slabs_in_flight);
  *cohort = c;
  return ED_OK;
}
ED_CATCH("ed_cohort_create")

ED_EXPORT void ed_cohort_destroy(ed_cohort* c)
{
  if (!c) return;
  (void)hipSetDevice(c->plan->device);
  (void)hipDeviceSynchronize();
  delete c;
}

// the reference point of the emission intervals: an event that has completed, on the cohort's device
static int cohort_epoch(ed_cohort* c)
{
  HIP_TRY(hipSetDevice(c->plan->device));
  if (!c->epoch) HIP_TRY(c->epoch.create());
  HIP_TRY(hipEventRecord(c->epoch, c->mains[0]));
  HIP_TRY(hipEventSynchronize(c->epoch));
  return ED_OK;
}

ED_EXPORT int ed_cohort_set_option(ed_cohort* c, const char* name, double value)
try {
  if (!c || !name) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option: NULL argument");
  const std::string k(name);
  if (k == "timing") {   // may change at any time
    c->timing = value != 0;
    c->emit_iv.clear();
    if (c->timing && c->started) { if (int rc = cohort_epoch(c)) return rc; }
    for (auto& sl : c->slots) {
      for (ed_batch* b : {sl.batch.get(), sl.odd.get()}) {
        if (!b) continue;
        ed_batch_enable_timing(b, c->timing);
        b->epoch = c->timing ? c->epoch.get() : nullptr; b->emit_iv = c->timing ? &c->emit_iv : nullptr;
      }
    }
    return ED_OK;
  }
  if (c->started) return ed_fail(ED_ERR_STATE, "ed_cohort_set_option(%s): options are fixed once the first slab has been submitted", name);
  if (k == "split") {
    if (!(value >= 0.0 && value < 1.0)) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(split): 0 <= value < 1");
    c->split_frac = value; c->split_set = true;
  } else if (k == "own_queues") c->own_queues = value != 0;
  else if (k == "fit_mode") {
    if (value != 0 && value != 1) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(fit_mode): 0 (maximum likelihood) or 1 (aod-nm)");
    c->fit_mode = (int)value;
  } else if (k == "phi_bins") {
    if (!(value == 1 || (value >= 2 && value <= kMaxPhiBins && value == (double)(int)value)))
      return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(phi_bins): 1 (one dispersion per sample) or 2..%d depth levels", kMaxPhiBins);
    c->phi_bins = (int)value;
  } else if (k == "bins_pieces") {
    if (!(value >= 1 && value <= 256)) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(bins_pieces): 1..256");
    c->bins_pieces = (int)value;
  } else if (k == "emit_mode") {
    if (value != 0 && value != 1 && value != 2) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(emit_mode): 0 (strict), 1 (tables) or 2 (tables, sample-major)");
    c->emit_mode = (int)value;
  } else if (k == "counts_layout") {
    if (value != 0 && value != 1) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(counts_layout): 0 ([n_exons][n_samples]) or 1 ([n_samples][n_exons])");
    c->counts_layout = (int)value;
  } else if (k == "counts_bits") {
    if (value != 32 && value != 16) return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(counts_bits): 32 (int32 device counts) or 16 (uint16; needs counts_layout 1 and emit_mode 2)");
    c->counts_bits = (int)value;
  } else if (k == "host_narrow") c->host_narrow = value != 0;
  else if (k == "emit_tails") c->emit_tails = value != 0;
  else if (k == "viterbi_overlap") c->viterbi_overlap = value != 0;
  else if (k == "tables_early") c->tables_early = value != 0;
  else if (k == "lanes") {
    if (!(value == 0 || (value >= 1 && value <= ed_cohort::kMaxLanes && value == (double)(int)value && c->n_slots % (int)value == 0)))
      return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option(lanes): 1..%d, a divisor of slabs_in_flight = %d, or 0 (slabs_in_flight / 2)", ed_cohort::kMaxLanes, c->n_slots);
    c->lanes_opt = (int)value;
  }
  else return ed_fail(ED_ERR_INVALID, "ed_cohort_set_option: unknown option '%s'", name);
  return ED_OK;
}
ED_CATCH("ed_cohort_set_option")

static int batch_make(std::unique_ptr<ed_batch>& out, ed_plan* plan, int64_t n)
{
  ed_batch* b = nullptr;
  if (int rc = ed_batch_create(&b, plan, n)) return rc;
  out.reset(b);
  return ED_OK;
}

// streams, slot buffers and the nominal batch objects: on the first submission, in a fixed order
static int cohort_start(ed_cohort* c)
{
  if (c->started) return ED_OK;
  const int dev = c->plan->device;
  HIP_TRY(hipSetDevice(dev));
  c->n_lanes = c->lanes_opt > 0 ? c->lanes_opt : ((c->n_slots >= 4 && c->n_slots % 2 == 0) ? std::min(c->n_slots / 2, (int)ed_cohort::kMaxLanes) : 1);   // (0: the automatic rule)
  if (c->n_slots % c->n_lanes) c->n_lanes = 1;
  const bool pipelined = c->pipelined();
  // (every resource is made only if it is not there yet: a start that failed half-way -- device memory -- is taken up where it stopped by the next
  // submission instead of making the streams, batch objects and buffers it already has a second time)
  for (int l = 0; l < c->n_lanes; ++l) {
    if (!c->mains[l]) HIP_TRY(ed_stream_create(c->mains[l], c->own_queues, dev));
    if (pipelined && !c->fits[l]) HIP_TRY(ed_stream_create(c->fits[l], c->own_queues, dev));
  }
  for (size_t i = 0; i < c->slots.size(); ++i) c->slots[i].lane = (int)(i % (size_t)c->n_lanes);
  for (auto& sl : c->slots) {
    if (!sl.batch) {
      if (int rc = batch_make(sl.batch, c->plan, c->slab)) return rc;
      if (c->own_queues && !sl.batch->sides.empty()) {   // the stream the chains run on (single-group mode uses the first side stream only)
        Stream own;
        HIP_TRY(ed_stream_create(own, true, dev));
        sl.batch->replace_side(0, std::move(own));
      }
    }
    if (!sl.d_phi) HIP_TRY(sl.d_phi.alloc((size_t)c->slab * 8));
    if (!sl.d_exp) HIP_TRY(sl.d_exp.alloc((size_t)c->slab * 8));
    if (c->phi_bins > 1) {
      if (!sl.d_phib) HIP_TRY(sl.d_phib.alloc((size_t)kMaxPhiBins * c->slab * 8));
      if (!sl.d_edges) HIP_TRY(sl.d_edges.alloc((size_t)(kMaxPhiBins + 1) * c->slab * 8));
    }
    if (!sl.emitted) HIP_TRY(sl.emitted.create(hipEventDisableTiming));
    if (!sl.fitted) HIP_TRY(sl.fitted.create(hipEventDisableTiming));
    if (!sl.ready) HIP_TRY(sl.ready.create(hipEventDisableTiming));
  }
  c->started = true;
  return ED_OK;
}

// pipeline settings of a batch object that serves this cohort
static int cohort_adopt(ed_cohort* c, ed_batch* b)
{
  const bool pipelined = c->pipelined();
  b->own_queues = c->own_queues;
  if (pipelined) {
    if (int rc = ed_batch_set_async_tail(b, 1)) return rc;
    if (int rc = ed_batch_set_viterbi_overlap(b, c->viterbi_overlap)) return rc;
    // (emit mode 2: no cut -- the sample-major fit's workgroups are small, the next slab's fit is issued as soon as its stream is free)
    if (!c->viterbi_overlap && c->split_frac > 0.0 && !(c->emit_mode == 2 && !c->split_set)) {
      if (!b->split_ev) HIP_TRY(b->split_ev.create(hipEventDisableTiming));
      b->split_frac = c->split_frac;
    }
  }
  // one slab at a time in the sample-major table mode: one emission launch, then the chains -- the overlap groups (chains of a chromosome
  // group under the emissions of the next) were made for the VALU-bound strict kernel; here the Viterbi waves' registers keep emission
  // workgroups off their CUs (a lone 200 000 x 1024 slab: 5.0 against 5.4 ms)
  if (!pipelined && c->emit_mode == 2 && c->phi_bins == 1) { if (int rc = ed_batch_set_viterbi_overlap(b, c->viterbi_overlap)) return rc; }
  b->fit_mode = c->fit_mode;
  b->counts_layout = c->counts_layout;
  b->counts_bits = c->counts_bits;
  b->tab_tails = c->emit_tails;
  if (b->emit_mode != (c->phi_bins > 1 ? 0 : c->emit_mode)) { if (int rc = ed_batch_set_emit_mode(b, c->phi_bins > 1 ? 0 : c->emit_mode)) return rc; }
  b->bins_pieces = (pipelined && c->phi_bins > 1) ? c->bins_pieces : 1;
  if (c->timing && !b->timing) ed_batch_enable_timing(b, 1);   // (enabling resets the sums: once per batch object)
  if (c->timing && !c->epoch) { if (int rc = cohort_epoch(c)) return rc; }
  b->epoch = c->timing ? c->epoch.get() : nullptr; b->emit_iv = c->timing ? &c->emit_iv : nullptr;
  return ED_OK;
}

// Depth-binned mode: the outcome of the slot's fit (issued blind by cohort_submit).  Converged on the histograms: nothing to do.
// An empty depth level: the reference's stop() -- the error of this ticket.  The histogram form declined (its emission kernels
// then returned at once) or a sample needs more passes: the slab is done again through the synchronous entries, which take the
// per-cell form / the rest of the pass budget; the counts must still be where they were (the caller's arrays until the ticket has
// been waited for, as documented; the slot's own for host-fed slabs).
static int cohort_bins_settle(ed_cohort* c, ed_cohort::Slot& sl)
{
  if (!sl.bins_pending) return ED_OK;
  sl.bins_pending = false;
  ed_batch* b = sl.cur;
  int status = 0;
  if (int rc = fit_bins_hist_status(b, c->phi_bins, &status)) return rc;
  if (status == 0) { b->bins_unconverged = 0; return ED_OK; }
  if (int rc = batch_ready(b)) return rc;
  hipStream_t main_st = c->mains[sl.lane];
  b->d_mix = sl.last_mix_s;
  if (int rc = ed_batch_fit_bins(b, sl.last_test, sl.last_ref, c->phi_bins, sl.d_phib, sl.d_edges, sl.d_exp, main_st)) return rc;
  if (int rc = ed_batch_run_bins(b, sl.last_test, sl.last_ref, c->phi_bins, sl.d_phib, sl.d_edges, sl.d_exp, sl.last_mix, main_st)) return rc;
  HIP_TRY(hipEventRecord(sl.emitted, main_st));
  return batch_ready(b);
}

// slab_bits: 0 = the cohort's option counts_bits; 16 / 32 = THIS slab's device counts are uint16 / int32 whatever the option says (host-fed slabs: the
// library itself chose the format of the slot's buffers).  d_mix: DEVICE double [n], one mixture per sample of the slab (NULL: `mixture` for all)
static int cohort_submit(ed_cohort* c, const int32_t* d_test, const int32_t* d_ref, int64_t n, const double* d_phi,
                         const double* d_expected, double mixture, hipStream_t ready_stream, int64_t* ticket, int slab_bits = 0,
                         const double* d_mix = nullptr)
{
  if (n <= 0 || n > c->slab) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit: %lld samples in a slab of %lld", (long long)n, (long long)c->slab);
  if ((d_phi == nullptr) != (d_expected == nullptr)) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit: phi and expected go together");
  if (c->counts_layout == 1 && (c->emit_mode != 2 || c->phi_bins > 1))
    return ed_fail(ED_ERR_STATE, "ed_cohort_submit: sample-major counts (option counts_layout = 1) need emit_mode = 2 and phi_bins = 1");
  if (c->counts_bits == 16 && c->counts_layout != 1)
    return ed_fail(ED_ERR_STATE, "ed_cohort_submit: 16-bit device counts (option counts_bits = 16) need counts_layout = 1 and emit_mode = 2");
  if (int rc = cohort_start(c)) return rc;
  HIP_TRY(hipSetDevice(c->plan->device));
  const int64_t t = c->next_ticket;
  ed_cohort::Slot& sl = c->slots[(size_t)(t % c->n_slots)];
  if (c->phi_bins > 1 && d_phi) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit: given (phi, expected) are per sample; with phi_bins > 1 the slab is fitted");
  if (int rc = cohort_bins_settle(c, sl)) return rc;   // (a ticket nobody waited for: its fit's workspace is about to be reused)
  ed_batch* b = sl.batch.get();
  if (n != c->slab) {
    if (sl.odd && sl.odd->S != n) {
      if (sl.cur == sl.odd.get()) { sl.cur = nullptr; sl.ticket = -1; }   // (the slot's last ticket dies with its batch: nothing may name it if the create below fails)
      sl.odd.reset();
    }
    if (!sl.odd) { if (int rc = batch_make(sl.odd, c->plan, n)) return rc; }
    b = sl.odd.get();
  }
  if (int rc = cohort_adopt(c, b)) return rc;
  if (slab_bits) b->counts_bits = slab_bits;
  b->d_mix = d_mix;   // (before batch_prepare below: the constants of this slab are made from it wherever they are made)
  const bool pipelined = c->pipelined();
  hipStream_t main_st = c->mains[sl.lane];                    // the slab's lane: its emission stream and its fit stream
  hipStream_t fit_st = pipelined ? c->fits[sl.lane] : main_st;
  // The slab's counts (and, when given, its parameters) are produced by work already enqueued on ready_stream: every stream of the lane that reads
  // them waits for it -- the emission stream, and in the pipelined form the fit stream, which carries the fit or, for given parameters, the
  // constants / table statistics / table build (batch_prepare).  Only a stream's wait for itself is left out: a producer on the cohort's own
  // emission stream (ed_cohort_stream) is ordered before that stream's work by stream order, but NOT before the fit stream's (ADVICE r5: the
  // event used to be skipped altogether for ready_stream == main_st).
  if (ready_stream != nullptr && (ready_stream != main_st || fit_st != main_st)) {
    HIP_TRY(hipEventRecord(sl.ready, ready_stream));
    if (ready_stream != main_st) HIP_TRY(hipStreamWaitEvent(main_st, sl.ready, 0));
    if (fit_st != main_st && ready_stream != fit_st) HIP_TRY(hipStreamWaitEvent(fit_st, sl.ready, 0));
  }
  // this slot's (phi, expected) are overwritten below: not before the emission kernels of the slot's previous run -- which
  // read the per-sample constants and tables made from them -- are through
  if (d_phi == nullptr) {
    if (pipelined && sl.emitted_set) HIP_TRY(hipStreamWaitEvent(fit_st, sl.emitted, 0));
    if (pipelined && t >= c->n_lanes) {
      // the issue point of this fit: inside the emission launch of the lane's previous slab (its split event)
      ed_cohort::Slot& prev = c->slots[(size_t)((t - c->n_lanes) % c->n_slots)];
      if (prev.cur && prev.cur->split_recorded) HIP_TRY(hipStreamWaitEvent(fit_st, prev.cur->split_ev, 0));
    }
    if (c->phi_bins > 1) {
      if (b->ran == false && b->d_loglik)   // (a declined fit leaves the chains the matrix as it is: defined values the first time too)
        HIP_TRY(hipMemsetAsync(b->d_loglik, 0, (size_t)std::max<int64_t>(c->plan->E, 1) * 3 * b->S * 8, fit_st));
      if (int rc = batch_fit_bins_async(b, d_test, d_ref, c->phi_bins, sl.d_phib, sl.d_edges, sl.d_exp, fit_st)) return rc;
    } else if (int rc = ed_batch_fit(b, d_test, d_ref, sl.d_phi, sl.d_exp, fit_st)) return rc;
    if (pipelined && c->tables_early && c->phi_bins == 1) { if (int rc = batch_prepare(b, sl.d_phi, sl.d_exp, mixture, fit_st, d_test, d_ref)) return rc; }
    if (pipelined) {
      HIP_TRY(hipEventRecord(sl.fitted, fit_st));
      HIP_TRY(hipStreamWaitEvent(main_st, sl.fitted, 0));
    }
  } else if (c->phi_bins == 1 && !b->fused) {
    // Given parameters (DEVICE arrays): k_sample_consts reads them where the caller has them and writes the slot's copy (two copies on the
    // emission stream before).  Pipelined: the constants and tables of the slab depend on nothing but these parameters and the counts, so
    // they are made on the fit stream -- underneath the previous slab's emissions -- and the emission stream carries the emission launch
    // alone (round 5: at 64 samples a slab the emission stream WAS the pipeline: 0.87 ms of copies, constants, table statistics, table
    // build and launch gaps around a 0.2 ms emission launch).  The slot's previous run must be through with the slot's arrays first.
    b->src_phi = d_phi; b->src_exp = d_expected;
    if (pipelined) {
      if (sl.emitted_set) HIP_TRY(hipStreamWaitEvent(fit_st, sl.emitted, 0));
      if (int rc = ed_batch_wait(b, fit_st)) return rc;        // (the tail of the batch's previous run reads its constants / decoration inputs)
      if (int rc = batch_prepare(b, sl.d_phi, sl.d_exp, mixture, fit_st, d_test, d_ref, true)) return rc;
      HIP_TRY(hipEventRecord(sl.fitted, fit_st));
      HIP_TRY(hipStreamWaitEvent(main_st, sl.fitted, 0));
    }
  } else {
    HIP_TRY(hipMemcpyAsync(sl.d_phi, d_phi, (size_t)n * 8, hipMemcpyDeviceToDevice, main_st));
    HIP_TRY(hipMemcpyAsync(sl.d_exp, d_expected, (size_t)n * 8, hipMemcpyDeviceToDevice, main_st));
  }
  if (c->phi_bins > 1) {
    if (int rc = batch_run_bins_skip(b, d_test, d_ref, c->phi_bins, sl.d_phib, sl.d_edges, sl.d_exp, mixture, main_st)) return rc;
    sl.bins_pending = true; sl.last_test = d_test; sl.last_ref = d_ref; sl.last_mix = mixture; sl.last_mix_s = d_mix;
  } else {
    const int rc = ed_batch_run(b, d_test, d_ref, sl.d_phi, sl.d_exp, mixture, main_st);
    b->src_phi = b->src_exp = nullptr;
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(sl.emitted, main_st));
  sl.emitted_set = true;
  sl.cur = b; sl.ticket = t; sl.n = n;
  ++c->next_ticket;
  if (ticket) *ticket = t;
  return ED_OK;
}

ED_EXPORT int ed_cohort_submit(ed_cohort* c, const int32_t* d_test, const int32_t* d_ref, int64_t n_samples, const double* d_phi,
                               const double* d_expected, double mixture, void* ready_stream, int64_t* ticket)
try {
  if (!c || !d_test || !d_ref) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit: NULL argument");
  return cohort_submit(c, d_test, d_ref, n_samples, d_phi, d_expected, mixture, (hipStream_t)ready_stream, ticket);
}
ED_CATCH("ed_cohort_submit")

ED_EXPORT int ed_cohort_submit_mix(ed_cohort* c, const int32_t* d_test, const int32_t* d_ref, int64_t n_samples, const double* d_phi,
                                   const double* d_expected, const double* d_mixture, void* ready_stream, int64_t* ticket)
try {
  if (!c || !d_test || !d_ref || !d_mixture) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_mix: NULL argument");
  return cohort_submit(c, d_test, d_ref, n_samples, d_phi, d_expected, 1.0, (hipStream_t)ready_stream, ticket, 0, d_mixture);
}
ED_CATCH("ed_cohort_submit_mix")

static int cohort_slot_of(ed_cohort* c, int64_t ticket, ed_cohort::Slot** out)
{
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  if (ticket < 0 || ticket >= c->next_ticket) return ed_fail(ED_ERR_INVALID, "ed_cohort: ticket %lld was never issued", (long long)ticket);
  ed_cohort::Slot& sl = c->slots[(size_t)(ticket % c->n_slots)];
  if (sl.ticket != ticket)
    return ed_fail(ED_ERR_STATE, "ed_cohort: the results of ticket %lld have been overwritten (only the last %d slabs are kept)",
                   (long long)ticket, c->n_slots);
  *out = &sl;
  return ED_OK;
}

ED_EXPORT int ed_cohort_batch(ed_cohort* c, int64_t ticket, ed_batch** batch, const double** d_phi, const double** d_expected)
try {
  ed_cohort::Slot* sl = nullptr;
  if (int rc = cohort_slot_of(c, ticket, &sl)) return rc;
  if (int rc = cohort_bins_settle(c, *sl)) return rc;
  if (batch) *batch = sl->cur;
  if (d_phi) *d_phi = sl->d_phi;
  if (d_expected) *d_expected = sl->d_exp;
  return ED_OK;
}
ED_CATCH("ed_cohort_batch")

// (phi, expected) of a ticket to host arrays, ordered on that slab's own stream (waits for that slab only)
ED_EXPORT int ed_cohort_copy_params(ed_cohort* c, int64_t ticket, double* phi_out, double* expected_out)
try {
  ed_cohort::Slot* sl = nullptr;
  if (int rc = cohort_slot_of(c, ticket, &sl)) return rc;
  if (int rc = cohort_bins_settle(c, *sl)) return rc;
  if (int rc = batch_ready(sl->cur)) return rc;
  if (c->phi_bins > 1 && phi_out) return ed_fail(ED_ERR_STATE, "ed_cohort_copy_params: with phi_bins > 1 the dispersions are per level (ed_cohort_copy_bins_params)");
  if (phi_out) { if (int rc = ed_d2h(phi_out, sl->d_phi, (size_t)sl->n * 8, sl->cur->stream)) return rc; }
  if (expected_out) { if (int rc = ed_d2h(expected_out, sl->d_exp, (size_t)sl->n * 8, sl->cur->stream)) return rc; }
  return ED_OK;
}
ED_CATCH("ed_cohort_copy_params")

ED_EXPORT int ed_cohort_wait(ed_cohort* c, int64_t ticket)
try {
  ed_cohort::Slot* sl = nullptr;
  if (int rc = cohort_slot_of(c, ticket, &sl)) return rc;
  if (int rc = cohort_bins_settle(c, *sl)) return rc;
  return batch_ready(sl->cur);
}
ED_CATCH("ed_cohort_wait")

// depth-binned mode: phi.estimates [phi_bins][n], complete.bins [(phi_bins + 1)][n] and fitted(mod) [n] of a ticket
ED_EXPORT int ed_cohort_copy_bins_params(ed_cohort* c, int64_t ticket, double* phi_bins_out, double* edges_out, double* expected_out)
try {
  ed_cohort::Slot* sl = nullptr;
  if (int rc = cohort_slot_of(c, ticket, &sl)) return rc;
  if (c->phi_bins < 2) return ed_fail(ED_ERR_STATE, "ed_cohort_copy_bins_params: the cohort runs the single-dispersion model (option phi_bins)");
  if (int rc = cohort_bins_settle(c, *sl)) return rc;
  if (int rc = batch_ready(sl->cur)) return rc;
  const int64_t n = sl->n;   // (the batch that served the ticket has exactly n samples: the arrays are [.][n])
  if (phi_bins_out) { if (int rc = ed_d2h(phi_bins_out, sl->d_phib, (size_t)c->phi_bins * n * 8, sl->cur->stream)) return rc; }
  if (edges_out) { if (int rc = ed_d2h(edges_out, sl->d_edges, (size_t)(c->phi_bins + 1) * n * 8, sl->cur->stream)) return rc; }
  if (expected_out) { if (int rc = ed_d2h(expected_out, sl->d_exp, (size_t)n * 8, sl->cur->stream)) return rc; }
  return ED_OK;
}
ED_CATCH("ed_cohort_copy_bins_params")

ED_EXPORT int ed_cohort_drain(ed_cohort* c)
try {
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  if (!c->started) return ED_OK;
  HIP_TRY(hipSetDevice(c->plan->device));
  for (auto& sl : c->slots)
    if (sl.cur) {
      if (int rc = cohort_bins_settle(c, sl)) return rc;
      if (int rc = batch_ready(sl.cur)) return rc;
    }
  for (int l = 0; l < c->n_lanes; ++l) {
    if (c->mains[l]) HIP_TRY(hipStreamSynchronize(c->mains[l]));
    if (c->fits[l]) HIP_TRY(hipStreamSynchronize(c->fits[l]));
  }
  if (c->copy) HIP_TRY(hipStreamSynchronize(c->copy));
  return ED_OK;
}
ED_CATCH("ed_cohort_drain")

ED_EXPORT void* ed_cohort_stream(ed_cohort* c)
{
  if (!c) return nullptr;
  if (cohort_start(c) != ED_OK) return nullptr;
  return (void*)c->mains[0];     // (lane 0's; a slab of another lane whose counts are made on it is ordered behind them through its `ready` event like any other stream's)
}

ED_EXPORT int ed_cohort_stage_ms_total(ed_cohort* c, double ms_total[5], int64_t* n_runs, int64_t* n_fits)
try {
  if (!c || !ms_total) return ed_fail(ED_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 5; ++i) ms_total[i] = 0.0;
  int64_t nr = 0, nf = 0;
  for (auto& sl : c->slots) {
    for (ed_batch* b : {sl.batch.get(), sl.odd.get()}) {
      if (!b) continue;
      double ms[5];
      int64_t r = 0, f = 0;
      if (int rc = ed_batch_stage_ms_total(b, ms, &r, &f)) return rc;
      for (int i = 0; i < 5; ++i) ms_total[i] += ms[i];
      nr += r; nf += f;
    }
  }
  if (n_runs) *n_runs = nr;
  if (n_fits) *n_fits = nf;
  return ED_OK;
}
ED_CATCH("ed_cohort_stage_ms_total")

// Option timing: the emission stage of every run folded since the option was set, as (start_ms, end_ms) pairs relative to one reference event -- the
// stages of different lanes run side by side, so a stage's own duration is not the chip's time for it; the union of these intervals is.
// out[2 * cap]; *n = pairs available (the first min(n, cap) are written).
ED_EXPORT int ed_cohort_emission_intervals(ed_cohort* c, float* out, int64_t cap, int64_t* n)
try {
  if (!c || !n || (cap > 0 && !out)) return ed_fail(ED_ERR_INVALID, "NULL argument");
  for (auto& sl : c->slots)
    for (ed_batch* b : {sl.batch.get(), sl.odd.get()}) { if (b) { if (int rc = fold_run_times(b)) return rc; } }
  *n = (int64_t)c->emit_iv.size() / 2;
  const int64_t k = std::min(*n, cap);
  if (k > 0) std::memcpy(out, c->emit_iv.data(), (size_t)k * 8);
  return ED_OK;
}
ED_CATCH("ed_cohort_emission_intervals")

ED_EXPORT int ed_cohort_n_emit_launches(ed_cohort* c)
try {
  if (!c) return 0;
  if (cohort_start(c) != ED_OK) return 0;
  if (c->phi_bins > 1)   // the tabulated-constants kernel in `bins_pieces` launches (one when nothing is in flight) + the per-cell kernel for what it left
    return (c->pipelined() ? c->bins_pieces : 1) + 1;
  if (cohort_adopt(c, c->slots[0].batch.get()) != ED_OK) return 0;
  return ed_batch_n_emit_launches(c->slots[0].batch.get());
}
ED_CATCH("ed_cohort_n_emit_launches")

// ---- host-fed slabs ----------------------------------------------------------------------------
// layout 0: host block is [E][n] sample-minor (the EDCOUNT1 container, exomedepth_amd/io.py); row_stride = elements between
//           consecutive exons in the host matrix (n for a dense slab, the cohort's width for a column window)
// layout 1: host block is R's E x n column-major matrix ([n][E]; a slab of columns is contiguous)
// wire 4: int32 elements; 2: uint16 elements (widened on the device)
static int upload_counts(ed_stager* g, hipStream_t st, const void* host, int64_t E, int64_t n, int layout, int wire, int64_t row_stride,
                         void* d_raw, int32_t* d_out, int phases, int dev_layout = 0);
static int cohort_upload_matrix(ed_cohort* c, ed_cohort::Slot& sl, const void* host, int64_t n, int layout, int wire,
                                int64_t row_stride, int which, int32_t* d_out, int phases)
{
  char* raw = sl.raw ? sl.raw + (size_t)which * (sl.raw.bytes() / 2) : nullptr;
  if (c->counts_layout == 1 && layout != 1)
    return ed_fail(ED_ERR_INVALID, "host-fed slabs of a cohort with counts_layout = 1 come in layout 1 (R's column-major matrix)");
  if (c->counts_bits == 16)
    return ed_fail(ED_ERR_STATE, "option counts_bits = 16 describes device-resident slabs (ed_cohort_submit); host-fed slabs choose their device format themselves "
                                 "(uint16 whenever the counts fit and the cohort runs sample-major tables)");
  return upload_counts(c->stager.get(), c->copy, host, c->plan->E, n, layout, wire, row_stride, raw, d_out, phases, c->counts_layout);
}

static int cohort_host_buffers(ed_cohort* c, ed_cohort::Slot& sl, bool need_raw)
{
  const int64_t E = c->plan->E;
  if (!c->copy) HIP_TRY(ed_stream_create(c->copy, c->own_queues, c->plan->device));
  if (!c->stager) { if (int rc = stager_make(c->stager, c->plan->device, (size_t)64 << 20)) return rc; }
  const size_t bytes = (size_t)std::max<int64_t>(E, 1) * c->slab * 4;
  if (!sl.own_test) HIP_TRY(sl.own_test.alloc(bytes));     // (each on its own owner: a failed second allocation is retried, not skipped)
  if (!sl.own_ref) HIP_TRY(sl.own_ref.alloc(bytes));
  if (need_raw && !sl.raw) HIP_TRY(sl.raw.alloc(2 * bytes));
  return ED_OK;
}

// One slab from host memory: both matrices through the copy stream, then cohort_submit.  The slot's device buffers are
// reused: the caller must have collected the results of ticket - slabs_in_flight (its decoration reads the counts).
static int cohort_submit_host(ed_cohort* c, const void* test, const void* ref, int64_t n_samples, int layout, int wire,
                              int64_t row_stride, const double* phi, const double* expected, double mixture, int64_t* ticket,
                              const double* d_mix)
{
  if (!c || !test || !ref) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host: NULL argument");
  if ((layout != 0 && layout != 1) || (wire != 4 && wire != 2)) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host: layout 0 / 1, wire 4 / 2");
  if (n_samples <= 0 || n_samples > c->slab) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host: %lld samples in a slab of %lld", (long long)n_samples, (long long)c->slab);
  if (layout == 0 && row_stride < n_samples) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host: row_stride below the slab's width");
  if (int rc = cohort_start(c)) return rc;
  HIP_TRY(hipSetDevice(c->plan->device));
  ed_cohort::Slot& sl = c->slots[(size_t)(c->next_ticket % c->n_slots)];
  if (int rc = cohort_bins_settle(c, sl)) return rc;   // (depth-binned mode: a slab done again reads the slot's counts -- before they are overwritten)
  const bool keep16 = c->counts_layout == 1 && layout == 1 && c->emit_mode == 2 && c->phi_bins == 1 && c->counts_bits != 16 && c->host_narrow;
  if (int rc = cohort_host_buffers(c, sl, (layout == 1 && c->counts_layout == 0) || (wire == 2 && !keep16))) return rc;
  // the slot's count buffers are still read by the tail of its previous run (call counts need nothing, but a decoration
  // requested later would): wait for that run on the copy stream
  if (sl.cur) { if (int rc = ed_batch_wait(sl.cur, c->copy)) return rc; }
  if (sl.emitted_set) HIP_TRY(hipStreamWaitEvent(c->copy, sl.emitted, 0));
  // Sample-major tables (emit mode 2 on [samples][exons] counts: what the R-level entry runs): the slab stays 16 bits wide on the device.  A uint16
  // host block goes up as it lies; an int32 block in pageable memory -- R's integer matrix -- is narrowed by the host threads that stage it (half the
  // bytes on the link, no widening pass on the device).  A count beyond 65 535 anywhere in the slab: the whole slab as int32, as before.
  if (keep16) {
    const size_t count = (size_t)c->plan->E * (size_t)n_samples;
    bool wide = false;
    if (wire == 2) {
      if (int rc = stager_upload(c->stager.get(), test, 1, count * 2, count * 2, sl.own_test, c->copy)) return rc;
      if (int rc = stager_upload(c->stager.get(), ref, 1, count * 2, count * 2, sl.own_ref, c->copy)) return rc;
    } else if (!host_block_is_pinned(test) && !host_block_is_pinned(ref)) {
      if (int rc = stager_upload_narrow(c->stager.get(), (const int32_t*)test, count, sl.own_test.as<uint16_t>(), c->copy, &wide)) return rc;
      if (!wide) { if (int rc = stager_upload_narrow(c->stager.get(), (const int32_t*)ref, count, sl.own_ref.as<uint16_t>(), c->copy, &wide)) return rc; }
      if (wide) ++c->n_wide_slabs;
    } else wide = true;                  // (pinned int32: the DMA engine reads it in place -- no host pass to narrow in)
    if (!wide) return cohort_submit(c, sl.own_test, sl.own_ref, n_samples, phi, expected, mixture, c->copy, ticket, 16, d_mix);
  }
  // both matrices onto the link first, then their device passes: the DMA engine is not left waiting behind a kernel
  if (int rc = cohort_upload_matrix(c, sl, test, n_samples, layout, wire, row_stride, 0, sl.own_test, 1)) return rc;
  if (int rc = cohort_upload_matrix(c, sl, ref, n_samples, layout, wire, row_stride, 1, sl.own_ref, 1)) return rc;
  if (int rc = cohort_upload_matrix(c, sl, test, n_samples, layout, wire, row_stride, 0, sl.own_test, 2)) return rc;
  if (int rc = cohort_upload_matrix(c, sl, ref, n_samples, layout, wire, row_stride, 1, sl.own_ref, 2)) return rc;
  return cohort_submit(c, sl.own_test, sl.own_ref, n_samples, phi, expected, mixture, c->copy, ticket, 32, d_mix);
}

ED_EXPORT int ed_cohort_submit_host(ed_cohort* c, const void* test, const void* ref, int64_t n_samples, int layout, int wire,
                                    int64_t row_stride, const double* phi, const double* expected, double mixture, int64_t* ticket)
try {
  return cohort_submit_host(c, test, ref, n_samples, layout, wire, row_stride, phi, expected, mixture, ticket, nullptr);
}
ED_CATCH("ed_cohort_submit_host")

// The same with only the TEST counts coming from the host: in the reference's workflow (vignette/vignette.Rnw:390-402) the reference
// of a sample is the sum of other samples of the same cohort -- made on the device by ed_cohort_select_reference_sets from counts
// that are uploaded once -- so the aggregate references need not cross the link at all.  d_ref: DEVICE int32 [n_exons][n_samples],
// complete when this is called (or ordered before the cohort's copy stream by the caller).
ED_EXPORT int ed_cohort_submit_host_test(ed_cohort* c, const void* test, const int32_t* d_ref, int64_t n_samples, int layout, int wire,
                                         int64_t row_stride, const double* phi, const double* expected, double mixture, int64_t* ticket)
try {
  if (!c || !test || !d_ref) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host_test: NULL argument");
  if ((layout != 0 && layout != 1) || (wire != 4 && wire != 2)) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host_test: layout 0 / 1, wire 4 / 2");
  if (n_samples <= 0 || n_samples > c->slab) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host_test: %lld samples in a slab of %lld", (long long)n_samples, (long long)c->slab);
  if (layout == 0 && row_stride < n_samples) return ed_fail(ED_ERR_INVALID, "ed_cohort_submit_host_test: row_stride below the slab's width");
  if (int rc = cohort_start(c)) return rc;
  HIP_TRY(hipSetDevice(c->plan->device));
  ed_cohort::Slot& sl = c->slots[(size_t)(c->next_ticket % c->n_slots)];
  if (int rc = cohort_bins_settle(c, sl)) return rc;   // (depth-binned mode: a slab done again reads the slot's counts -- before they are overwritten)
  if (int rc = cohort_host_buffers(c, sl, layout == 1 || wire == 2)) return rc;
  if (sl.cur) { if (int rc = ed_batch_wait(sl.cur, c->copy)) return rc; }
  if (sl.emitted_set) HIP_TRY(hipStreamWaitEvent(c->copy, sl.emitted, 0));
  if (int rc = cohort_upload_matrix(c, sl, test, n_samples, layout, wire, row_stride, 0, sl.own_test, 3)) return rc;
  return cohort_submit(c, sl.own_test, d_ref, n_samples, phi, expected, mixture, c->copy, ticket);
}
ED_CATCH("ed_cohort_submit_host_test")

ED_EXPORT int ed_cohort_ingest_stats(ed_cohort* c, double* bytes, double* host_seconds)
try {
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  if (bytes) *bytes = c->stager ? c->stager->bytes : 0.0;
  if (host_seconds) *host_seconds = c->stager ? c->stager->seconds_host : 0.0;
  return ED_OK;
}
ED_CATCH("ed_cohort_ingest_stats")

ED_EXPORT int ed_cohort_n_wide_slabs(ed_cohort* c, int64_t* n)
try {
  if (!c || !n) return ed_fail(ED_ERR_INVALID, "NULL argument");
  *n = c->n_wide_slabs;
  return ED_OK;
}
ED_CATCH("ed_cohort_n_wide_slabs")

// Results of one ticket into the cohort's host-side table: calls (sample indices shifted to the cohort's axis), their
// decoration, and on request the fitted parameters and the path.
static int cohort_collect(ed_cohort* c, int64_t ticket, int64_t sample0, int64_t S_total, int layout, double* phi_out,
                          double* expected_out, uint8_t* path_out, bool want_info)
{
  ed_cohort::Slot* slp = nullptr;
  if (int rc = cohort_slot_of(c, ticket, &slp)) return rc;
  ed_cohort::Slot& sl = *slp;
  if (int rc = cohort_bins_settle(c, sl)) return rc;
  ed_batch* b = sl.cur;
  const int64_t E = c->plan->E, n = sl.n;
  if (c->phi_bins > 1) {   // per-level dispersions and edges of the slab into the cohort-wide host arrays
    const int B = c->phi_bins;
    std::vector<double> tmp((size_t)(2 * B + 1) * n);
    if (int rc = batch_ready(b)) return rc;
    if (int rc = ed_d2h(tmp.data(), sl.d_phib, (size_t)B * n * 8, b->stream)) return rc;
    if (int rc = ed_d2h(tmp.data() + (size_t)B * n, sl.d_edges, (size_t)(B + 1) * n * 8, b->stream)) return rc;
    for (int g = 0; g < B; ++g) std::memcpy(&c->h_phib[(size_t)g * S_total + sample0], &tmp[(size_t)g * n], (size_t)n * 8);
    for (int g = 0; g <= B; ++g) std::memcpy(&c->h_edges[(size_t)g * S_total + sample0], &tmp[(size_t)(B + g) * n], (size_t)n * 8);
    phi_out = nullptr;   // (per sample there is none)
  }
  int64_t k = 0;
  if (int rc = ed_batch_n_calls(b, &k)) return rc;
  const size_t at = c->calls.size();
  c->calls.resize(at + (size_t)k);
  if (int rc = ed_batch_copy_calls(b, c->calls.data() + at, k)) return rc;
  for (size_t i = at; i < c->calls.size(); ++i) c->calls[i].sample += (int32_t)sample0;
  if (want_info) {
    c->info.resize(at + (size_t)k);
    if (int rc = ed_batch_copy_call_info(b, c->info.data() + at, k)) return rc;
  }
  int64_t ne = 0;
  if (int rc = ed_batch_n_gsl_errors(b, &ne)) return rc;
  c->n_gsl_errors += ne;
  {
    int64_t ts[4];
    if (int rc = ed_batch_table_stats(b, ts)) return rc;
    for (int i = 0; i < 4; ++i) c->tab_stats[i] += ts[i];
  }
  if (phi_out) { if (int rc = ed_d2h(phi_out + sample0, sl.d_phi, (size_t)n * 8, b->stream)) return rc; }
  if (expected_out) { if (int rc = ed_d2h(expected_out + sample0, sl.d_exp, (size_t)n * 8, b->stream)) return rc; }
  if (path_out && E > 0) {
    if (int rc = ensure_path(b)) return rc;
    if (layout == 1) {
      if (!sl.path_cols) HIP_TRY(sl.path_cols.alloc((size_t)E * c->slab));
      hipLaunchKernelGGL(k_rows_to_cols<uint8_t>, dim3((unsigned)((E + 63) / 64), (unsigned)((n + 63) / 64)), dim3(256), 0, b->stream, (const uint8_t*)b->d_path, E, n,
                         sl.path_cols);
      HIP_TRY(hipGetLastError());
      if (int rc = ed_d2h(path_out + (size_t)sample0 * E, sl.path_cols, (size_t)E * n, b->stream)) return rc;
    } else {
      HIP_TRY(hipMemcpy2DAsync(path_out + sample0, (size_t)S_total, b->d_path, (size_t)n, (size_t)n, (size_t)E, hipMemcpyDeviceToHost, b->stream));
      HIP_TRY(hipStreamSynchronize(b->stream));
    }
  }
  return ED_OK;
}

// CallCNVs for a whole cohort held in host memory: cut into slabs, pipelined (upload of slab t+1 || compute of slab t ||
// collection of slab t-1).  See include/exomedepth_amd.h.
// The slabs come from `next_slab` (slab i = columns [i slab, min((i + 1) slab, S_total)); < 0: no more): a counter for ed_cohort_run_host, the
// devices' shared queue for ed_multi_run_host (edmulti.inc).  Outputs go to their positions in the whole cohort, call rows are numbered by column
// of the whole cohort; `segs` (optional) receives, per collected slab, (slab, first row, end row) in c->calls / c->info.
struct ed_slab_seg { int64_t slab, row0, row1; };
template <class NEXT>
static int cohort_run_host_slabs(ed_cohort* c, const void* test, const void* ref, int64_t S_total, NEXT next_slab, int layout, int wire,
                                 const double* phi, const double* expected, double mixture, const double* mix_host, double* phi_out,
                                 double* expected_out, uint8_t* path_out, int64_t* n_calls, std::vector<ed_slab_seg>* segs)
{
  if (!c || !test || !ref || S_total <= 0) return ed_fail(ED_ERR_INVALID, "ed_cohort_run_host: bad arguments");
  if ((phi == nullptr) != (expected == nullptr)) return ed_fail(ED_ERR_INVALID, "ed_cohort_run_host: phi and expected go together");
  const int64_t E = c->plan->E;
  c->calls.clear(); c->info.clear(); c->n_unconverged = 0; c->n_gsl_errors = 0;
  if (segs) segs->clear();
  for (int i = 0; i < 4; ++i) c->tab_stats[i] = 0;
  if (c->phi_bins > 1) {
    if (phi) return ed_fail(ED_ERR_INVALID, "ed_cohort_run_host: given (phi, expected) are per sample; with phi_bins > 1 every slab is fitted");
    c->h_phib.assign((size_t)c->phi_bins * S_total, 0.0);
    c->h_edges.assign((size_t)(c->phi_bins + 1) * S_total, 0.0);
  }
  struct Flight { int64_t ticket, slab; };
  std::vector<Flight> flight;                      // oldest first
  bool started = false;
  auto start = [&]() -> int {
    if (started) return ED_OK;
    if (int rc = cohort_start(c)) return rc;
    HIP_TRY(hipSetDevice(c->plan->device));
    if (!c->copy) HIP_TRY(ed_stream_create(c->copy, c->own_queues, c->plan->device));
    // given parameters: the whole vectors go to the device once (a pageable per-slab copy on the main stream would make the
    // host wait for that stream every time); the slabs then take their windows device to device
    if (phi) {
      HIP_TRY(c->d_par.reserve((size_t)S_total * 16));
      HIP_TRY(hipMemcpyAsync(c->d_par, phi, (size_t)S_total * 8, hipMemcpyHostToDevice, c->copy));
      HIP_TRY(hipMemcpyAsync(c->d_par + S_total, expected, (size_t)S_total * 8, hipMemcpyHostToDevice, c->copy));
      HIP_TRY(hipStreamSynchronize(c->copy));
    }
    // per-sample mixtures: the same way, complete on the device before any slab's constants kernel, on whichever stream that runs
    if (mix_host) {
      HIP_TRY(c->d_mixv.reserve((size_t)S_total * 8));
      HIP_TRY(hipMemcpyAsync(c->d_mixv, mix_host, (size_t)S_total * 8, hipMemcpyHostToDevice, c->copy));
      HIP_TRY(hipStreamSynchronize(c->copy));
    }
    started = true;
    return ED_OK;
  };
  auto collect = [&](const Flight& f) -> int {
    const int64_t s0 = f.slab * c->slab;
    const int64_t row0 = (int64_t)c->calls.size();
    if (int rc = cohort_collect(c, f.ticket, s0, S_total, layout, phi_out, expected_out, path_out, true)) return rc;
    if (segs) segs->push_back({f.slab, row0, (int64_t)c->calls.size()});
    if (phi == nullptr) {   // convergence of the slab's fit (the reference exposes optim()'s code the same way)
      ed_cohort::Slot* sl = nullptr;
      if (int rc = cohort_slot_of(c, f.ticket, &sl)) return rc;
      int64_t nu = 0;
      if (c->phi_bins > 1) {   // the depth-binned Newton's own flags (settled by the collect above), not the starting fit's
        if (int rc = ed_batch_fit_bins_n_unconverged(sl->cur, &nu)) return rc;
      } else {
        if (int rc = ed_batch_fit_n_unconverged(sl->cur, &nu, nullptr)) return rc;
      }
      c->n_unconverged += nu;
    }
    return ED_OK;
  };
  for (;;) {
    const int64_t i = next_slab();
    if (i < 0) break;
    if (int rc = start()) return rc;              // (a device that never gets a slab allocates nothing)
    const int64_t s0 = i * c->slab, n = std::min(c->slab, S_total - s0);
    if (s0 < 0 || n <= 0) return ed_fail(ED_ERR_STATE, "ed_cohort_run_host: slab %lld outside the cohort", (long long)i);
    if ((int)flight.size() >= c->n_slots) {       // frees the slot this slab goes into
      if (int rc = collect(flight.front())) return rc;
      flight.erase(flight.begin());
    }
    const size_t off = (layout == 1) ? (size_t)s0 * E * wire : (size_t)s0 * wire;
    int64_t tk = -1;
    if (int rc = cohort_submit_host(c, (const char*)test + off, (const char*)ref + off, n, layout, wire, S_total,
                                    phi ? c->d_par + s0 : nullptr, phi ? c->d_par + S_total + s0 : nullptr, mixture, &tk,
                                    mix_host ? c->d_mixv + s0 : nullptr))
      return rc;
    flight.push_back({tk, i});
  }
  for (const Flight& f : flight) { if (int rc = collect(f)) return rc; }
  if (n_calls) *n_calls = (int64_t)c->calls.size();
  return ED_OK;
}

ED_EXPORT int ed_cohort_run_host(ed_cohort* c, const void* test, const void* ref, int64_t S_total, int layout, int wire,
                                 const double* phi, const double* expected, double mixture, double* phi_out, double* expected_out,
                                 uint8_t* path_out, int64_t* n_calls)
try {
  if (!c || S_total <= 0) return ed_fail(ED_ERR_INVALID, "ed_cohort_run_host: bad arguments");
  const int64_t n_slabs = (S_total + c->slab - 1) / c->slab;
  int64_t i = 0;
  auto next = [&]() -> int64_t { return i < n_slabs ? i++ : -1; };
  return cohort_run_host_slabs(c, test, ref, S_total, next, layout, wire, phi, expected, mixture, nullptr, phi_out, expected_out, path_out, n_calls,
                               nullptr);
}
ED_CATCH("ed_cohort_run_host")

// host mixtures [n]: every one finite (ed_cohort_run_host_mix, ed_multi_run_host_mix) -- checked before anything is uploaded or launched
static int check_host_mixtures(const double* mixture, int64_t n, const char* who)
{
  if (!mixture) return ed_fail(ED_ERR_INVALID, "%s: NULL mixture", who);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(mixture[i])) return ed_fail(ED_ERR_INVALID, "%s: mixture of sample %lld is not a finite number", who, (long long)i);
  return ED_OK;
}

ED_EXPORT int ed_cohort_run_host_mix(ed_cohort* c, const void* test, const void* ref, int64_t S_total, int layout, int wire,
                                     const double* phi, const double* expected, const double* mixture, double* phi_out, double* expected_out,
                                     uint8_t* path_out, int64_t* n_calls)
try {
  if (!c || S_total <= 0) return ed_fail(ED_ERR_INVALID, "ed_cohort_run_host_mix: bad arguments");
  if (int rc = check_host_mixtures(mixture, S_total, "ed_cohort_run_host_mix")) return rc;
  const int64_t n_slabs = (S_total + c->slab - 1) / c->slab;
  int64_t i = 0;
  auto next = [&]() -> int64_t { return i < n_slabs ? i++ : -1; };
  return cohort_run_host_slabs(c, test, ref, S_total, next, layout, wire, phi, expected, 1.0, mixture, phi_out, expected_out, path_out, n_calls,
                               nullptr);
}
ED_CATCH("ed_cohort_run_host_mix")

ED_EXPORT int ed_cohort_copy_calls(ed_cohort* c, ed_call* calls, ed_call_info* info, int64_t cap)
try {
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  const int64_t k = std::min<int64_t>(cap, (int64_t)c->calls.size());
  if (k > 0 && calls) std::memcpy(calls, c->calls.data(), (size_t)k * sizeof(ed_call));
  if (k > 0 && info && c->info.size() >= (size_t)k) std::memcpy(info, c->info.data(), (size_t)k * sizeof(ed_call_info));
  return ED_OK;
}
ED_CATCH("ed_cohort_copy_calls")

// depth-binned mode, after ed_cohort_run_host: phi.estimates [phi_bins][S_total] and complete.bins [(phi_bins + 1)][S_total]
ED_EXPORT int ed_cohort_copy_bins(ed_cohort* c, double* phi_bins_out, double* edges_out)
try {
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  if (c->phi_bins < 2 || c->h_phib.empty()) return ed_fail(ED_ERR_STATE, "ed_cohort_copy_bins: no depth-binned run to report");
  if (phi_bins_out) std::memcpy(phi_bins_out, c->h_phib.data(), c->h_phib.size() * 8);
  if (edges_out) std::memcpy(edges_out, c->h_edges.data(), c->h_edges.size() * 8);
  return ED_OK;
}
ED_CATCH("ed_cohort_copy_bins")

ED_EXPORT int ed_cohort_run_status(ed_cohort* c, int64_t* n_unconverged, int64_t* n_gsl_errors)
try {
  if (!c) return ed_fail(ED_ERR_INVALID, "NULL cohort");
  if (n_unconverged) *n_unconverged = c->n_unconverged;
  if (n_gsl_errors) *n_gsl_errors = c->n_gsl_errors;
  return ED_OK;
}
ED_CATCH("ed_cohort_run_status")

// table-driven emit modes, after ed_cohort_run_host: ed_batch_table_stats summed over the cohort's slabs
ED_EXPORT int ed_cohort_table_status(ed_cohort* c, int64_t out[4])
try {
  if (!c || !out) return ed_fail(ED_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 4; ++i) out[i] = c->tab_stats[i];
  return ED_OK;
}
ED_CATCH("ed_cohort_table_status")

// ---- host-level entries behind the R wrappers of shim/edcore_shim.c ------------------------------
// upload a count matrix (layout / wire as ed_cohort_submit_host) to a dense device [E][n] int32 matrix, through `g` on `st`
// phases: 1 = the copy onto the link only, 2 = the device pass (widen / transpose) only, 3 = both.  A caller with several matrices
// issues all the copies first so that the DMA engine is not left idle behind a device pass.
static int upload_counts(ed_stager* g, hipStream_t st, const void* host, int64_t E, int64_t n, int layout, int wire, int64_t row_stride,
                         void* d_raw, int32_t* d_out, int phases, int dev_layout)
{
  if (layout == 1 && dev_layout == 1) {   // R's column-major matrix IS the sample-major device layout: no transposition
    void* dst = (wire == 4) ? (void*)d_out : d_raw;
    if (phases & 1) { if (int rc = stager_upload(g, host, 1, (size_t)E * n * wire, (size_t)E * n * wire, dst, st)) return rc; }
    if ((phases & 2) && wire == 2)
      hipLaunchKernelGGL(k_widen_u16, dim3((unsigned)std::min<int64_t>((E * n + 255) / 256, 65535)), dim3(256), 0, st, (const uint16_t*)d_raw, E * n, d_out);
  } else if (layout == 0) {
    void* dst = (wire == 4) ? (void*)d_out : d_raw;
    if (phases & 1) { if (int rc = stager_upload(g, host, (size_t)E, (size_t)n * wire, (size_t)row_stride * wire, dst, st)) return rc; }
    if ((phases & 2) && wire == 2)
      hipLaunchKernelGGL(k_widen_u16, dim3((unsigned)std::min<int64_t>((E * n + 255) / 256, 65535)), dim3(256), 0, st, (const uint16_t*)d_raw, E * n, d_out);
  } else {
    if (phases & 1) { if (int rc = stager_upload(g, host, 1, (size_t)E * n * wire, (size_t)E * n * wire, d_raw, st)) return rc; }
    if (phases & 2) {
      const dim3 grid((unsigned)((E + 63) / 64), (unsigned)((n + 63) / 64));
      if (wire == 4) hipLaunchKernelGGL(k_cols_to_rows<int32_t>, grid, dim3(256), 0, st, (const int32_t*)d_raw, E, n, d_out);
      else hipLaunchKernelGGL(k_cols_to_rows<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)d_raw, E, n, d_out);
    }
  }
  HIP_TRY(hipGetLastError());
  return ED_OK;
}
static int upload_counts(ed_stager* g, hipStream_t st, const void* host, int64_t E, int64_t n, int layout, int wire, int64_t row_stride,
                         void* d_raw, int32_t* d_out)
{
  return upload_counts(g, st, host, E, n, layout, wire, row_stride, d_raw, d_out, 3);
}

// The model fit of new('ExomeDepth') alone -- what stands where aod::betabin is called (reference R/class_definition.R:118,
// :168) -- for every column of a host-resident cohort.
ED_EXPORT int ed_fit_betabin_host(const void* test, const void* ref, int64_t n_exons, int64_t n_samples, int layout, int wire,
                                  int fit_mode, double* phi_out, double* expected_out, int32_t* converged_out)
try {
  if (!test || !ref || !phi_out || !expected_out || n_exons <= 0 || n_samples <= 0)
    return ed_fail(ED_ERR_INVALID, "ed_fit_betabin_host: bad arguments");
  if ((layout != 0 && layout != 1) || (wire != 4 && wire != 2)) return ed_fail(ED_ERR_INVALID, "ed_fit_betabin_host: layout 0 / 1, wire 4 / 2");
  if (int rc = require_device()) return rc;
  const int64_t E = n_exons, slab = std::min<int64_t>(n_samples, 1024);
  // a plan only carries the exon count here: one chromosome, unit positions
  std::vector<int32_t> off = {0, (int32_t)E}, st((size_t)E), en((size_t)E);
  for (int64_t i = 0; i < E; ++i) { st[(size_t)i] = (int32_t)i; en[(size_t)i] = (int32_t)i + 1; }
  ed_plan* plan = nullptr;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (int rc = ed_plan_create(&plan, dev, E, 1, off.data(), st.data(), en.data(), 1e-4, 5e4)) return rc;
  struct Work {      // (members go in reverse order: the feed first, then the batches, the plan, the buffers)
    DevBuf<void> t, r, raw, phi, ex;
    std::unique_ptr<ed_plan> plan; std::unique_ptr<ed_batch> odd, b; HostFeed f;
  } k;
  k.plan.reset(plan);
  if (int rc = k.f.open(dev)) return rc;
  HIP_TRY(k.t.alloc((size_t)E * slab * 4)); HIP_TRY(k.r.alloc((size_t)E * slab * 4));
  HIP_TRY(k.raw.alloc((size_t)E * slab * 4));
  HIP_TRY(k.phi.alloc((size_t)slab * 8)); HIP_TRY(k.ex.alloc((size_t)slab * 8));
  for (int64_t s0 = 0; s0 < n_samples; s0 += slab) {
    const int64_t n = std::min(slab, n_samples - s0);
    std::unique_ptr<ed_batch>& b = (n == slab) ? k.b : k.odd;
    if (!b) { if (int rc = batch_make(b, plan, n)) return rc; b->fit_mode = fit_mode; }
    const size_t off_b = (layout == 1) ? (size_t)s0 * E * wire : (size_t)s0 * wire;
    if (int rc = upload_counts(k.f.g.get(), k.f.s, (const char*)test + off_b, E, n, layout, wire, n_samples, k.raw.get(), k.t.as<int32_t>())) return rc;
    if (int rc = upload_counts(k.f.g.get(), k.f.s, (const char*)ref + off_b, E, n, layout, wire, n_samples, k.raw.get(), k.r.as<int32_t>())) return rc;
    if (int rc = ed_batch_fit(b.get(), k.t.as<int32_t>(), k.r.as<int32_t>(), k.phi.as<double>(), k.ex.as<double>(), k.f.s)) return rc;
    if (int rc = ed_d2h(phi_out + s0, k.phi.get(), (size_t)n * 8, k.f.s)) return rc;
    if (int rc = ed_d2h(expected_out + s0, k.ex.get(), (size_t)n * 8, k.f.s)) return rc;
    if (converged_out) { if (int rc = ed_d2h(converged_out + s0, b->fitw->done, (size_t)n * 4, k.f.s)) return rc; }
  }
  return ED_OK;
}
ED_CATCH("ed_fit_betabin_host")

// select.reference.set (reference R/optimize_reference_set.R:53-148) on host data in R's layout: test.counts integer[n_bins],
// reference.counts the n_bins x n_refs integer matrix, column-major.
ED_EXPORT int ed_select_reference_set_host(const int32_t* test, const int32_t* refs_colmajor, int64_t n_bins, int64_t n_refs,
                                           const double* bin_length, int64_t n_bins_reduced, ed_refset_row* rows, int32_t* n_chosen,
                                           int64_t* n_selected_bins)
try {
  if (!test || !refs_colmajor || !rows || !n_chosen || n_bins <= 0 || n_refs <= 0)
    return ed_fail(ED_ERR_INVALID, "ed_select_reference_set_host: bad arguments");
  if (int rc = require_device()) return rc;
  int dev = 0;
  (void)hipGetDevice(&dev);
  struct Work { DevBuf<void> t, r, raw; HostFeed f; } k;      // (the feed goes before the buffers)
  if (int rc = k.f.open(dev)) return rc;
  HIP_TRY(k.t.alloc((size_t)n_bins * 4)); HIP_TRY(k.r.alloc((size_t)n_bins * n_refs * 4)); HIP_TRY(k.raw.alloc((size_t)n_bins * n_refs * 4));
  if (int rc = stager_upload(k.f.g.get(), test, 1, (size_t)n_bins * 4, (size_t)n_bins * 4, k.t.get(), k.f.s)) return rc;
  if (int rc = upload_counts(k.f.g.get(), k.f.s, refs_colmajor, n_bins, n_refs, 1, 4, n_refs, k.raw.get(), k.r.as<int32_t>())) return rc;
  HIP_TRY(hipStreamSynchronize(k.f.s));
  return ed_select_reference_set(k.t.as<int32_t>(), k.r.as<int32_t>(), n_bins, n_refs, bin_length, n_bins_reduced, rows, n_chosen,
                                 n_selected_bins, k.f.s);
}
ED_CATCH("ed_select_reference_set_host")
