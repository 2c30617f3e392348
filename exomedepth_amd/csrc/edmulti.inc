// edmulti.inc -- one host process, several devices.  Included by edcore.hip.
//
// The reference's user loops over the samples of a cohort in ONE R process (vignette/vignette.Rnw:390-431; per sample
// R/class_definition.R:82-191 + :311-419), and the samples are independent: no exchange step anywhere on the path.  So the
// multi-device form of CallCNVs-for-a-cohort needs no collective and no second process: the exon design (plan) is replicated on
// every device, the cohort's slabs sit in one queue, one host thread per device drives an ordinary cohort pipeline (edcohort.inc) over the
// slabs it takes from it -- reading the caller's host matrices in place and writing its windows of the caller's outputs -- and the compact
// call tables are put together in slab order, which IS the order of the columns.
// This is what the R-level entry edr_call_cnvs_batch (shim/edcore_shim.c) runs on: every visible device by default.
// exomedepth_amd/dist.py (one process per device, torch.distributed, one gather of the call tables over RCCL) stays the other
// N > 1 driver, for callers that already live in that world.
//
// The same device may be named more than once (devices = {0, 0}: two pipelines on one GPU) -- how the tests exercise the threads
// and the merge on a single-GPU box.

struct ed_multi {
  struct Dev {
    int device = 0;
    ed_plan* plan = nullptr;
    ed_cohort* cohort = nullptr;
    std::vector<ed_slab_seg> segs;      // the slabs this device's thread took in the last run, with their rows in its cohort's call table
    int64_t n_columns = 0;              // ... and how many columns they hold
    int rc = ED_OK;
    std::string err;
    double seconds = 0.0;               // wall time of the device's thread in the last run
    int numa_node = -1;                 // of the device (sysfs), -1 unknown: its host thread is kept on that node's CPUs
  };
  std::vector<Dev> devs;
  int64_t slab = 0;
  int phi_bins = 1;
  bool numa_bind = true;
  int64_t S_total = 0;                  // of the last run
  std::vector<ed_call> calls;
  std::vector<ed_call_info> info;
};

ED_EXPORT void ed_multi_destroy(ed_multi* m)
{
  if (!m) return;
  for (auto& d : m->devs) {
    if (d.cohort) ed_cohort_destroy(d.cohort);
    if (d.plan) ed_plan_destroy(d.plan);
  }
  delete m;
}

// NUMA node of a device: /sys/bus/pci/devices/<bus id>/numa_node (-1 when the platform does not say)
static int multi_numa_node_of(int device)
{
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
  for (char* q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}

// The calling thread onto the CPUs of a NUMA node (/sys/devices/system/node/nodeN/cpulist, e.g. "0-31,128-159"): the thread that stages a device's
// slabs -- and the copy threads it starts, which inherit its mask -- then read the caller's matrices and write the pinned staging buffers from the
// socket the device hangs on.  Best effort: any failure leaves the thread where it was.
static void multi_bind_thread_to_node(int node)
{
  if (node < 0) return;
  char path[96];
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  FILE* f = fopen(path, "r");
  if (!f) return;
  char buf[4096] = {0};
  const size_t got = fread(buf, 1, sizeof buf - 1, f);
  fclose(f);
  if (got == 0) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  int n_set = 0;
  for (const char* q = buf; *q;) {
    char* e = nullptr;
    const long a = strtol(q, &e, 10);
    if (e == q) break;
    long z = a;
    q = e;
    if (*q == '-') { z = strtol(q + 1, &e, 10); if (e == q + 1) break; q = e; }
    for (long k = a; k <= z && k < CPU_SETSIZE; ++k) { if (k >= 0) { CPU_SET((int)k, &set); ++n_set; } }
    while (*q == ',' || *q == '\n' || *q == ' ') ++q;
  }
  if (n_set > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
}

ED_EXPORT int ed_multi_create(ed_multi** multi, const int* devices, int n_devices, int64_t n_exons, int32_t n_chrom, const int32_t* chrom_off,
                              const int32_t* start, const int32_t* end, double transition_probability, double expected_cnv_length,
                              int64_t slab_samples, int slabs_in_flight)
try {
  if (!multi || n_devices < 0 || n_devices > 64 || slab_samples <= 0) return ed_fail(ED_ERR_INVALID, "ed_multi_create: bad arguments");
  const int visible = ed_device_count();
  if (visible <= 0) return ed_fail(ED_ERR_NO_DEVICE, "ed_multi_create: no HIP device is visible");
  // (owned here until it is handed over: whatever throws or fails below -- the vectors, a plan's host tables -- the devices' objects made so far go with it)
  struct Holder { ed_multi* m; ~Holder() { if (m) ed_multi_destroy(m); } } hold{new (std::nothrow) ed_multi};
  ed_multi* m = hold.m;
  if (!m) return ed_fail(ED_ERR_NOMEM, "out of host memory");
  const int n = (n_devices == 0 || !devices) ? visible : n_devices;     // default: every visible device once
  m->devs.resize((size_t)n);
  m->slab = slab_samples;
  for (int i = 0; i < n; ++i) {
    ed_multi::Dev& d = m->devs[(size_t)i];
    d.device = (n_devices == 0 || !devices) ? i : devices[i];
    if (d.device < 0 || d.device >= visible) return ed_fail(ED_ERR_INVALID, "ed_multi_create: device %d of %d visible", d.device, visible);
    if (int rc = ed_plan_create(&d.plan, d.device, n_exons, n_chrom, chrom_off, start, end, transition_probability, expected_cnv_length)) return rc;
    if (int rc = ed_cohort_create(&d.cohort, d.plan, slab_samples, slabs_in_flight)) return rc;
    d.numa_node = multi_numa_node_of(d.device);
  }
  hold.m = nullptr;
  *multi = m;
  return ED_OK;
}
ED_CATCH("ed_multi_create")

ED_EXPORT int ed_multi_n_devices(const ed_multi* m) { return m ? (int)m->devs.size() : 0; }

// every device's cohort takes the option (ed_cohort_set_option); "numa_bind" (1 default / 0) is the driver's own
ED_EXPORT int ed_multi_set_option(ed_multi* m, const char* name, double value)
try {
  if (!m || !name) return ed_fail(ED_ERR_INVALID, "ed_multi_set_option: NULL argument");
  if (std::string(name) == "numa_bind") { m->numa_bind = value != 0; return ED_OK; }
  for (auto& d : m->devs) { if (int rc = ed_cohort_set_option(d.cohort, name, value)) return rc; }
  if (std::string(name) == "phi_bins") m->phi_bins = (int)value;
  return ED_OK;
}
ED_CATCH("ed_multi_set_option")

// ed_cohort_run_host over every device.  The slabs are dealt from ONE queue (an atomic counter): a device's thread takes the next slab whenever a slot
// of its pipeline is free, so a device that is slower -- or busy with somebody else's work -- takes fewer slabs instead of setting the wall time with a
// fixed share (round 5 dealt contiguous shares).  Which device served a slab does not show in the results: every slab is fitted and called on its own, and
// the call table is put together in slab order = column order.
static int multi_run_host(ed_multi* m, const void* test, const void* ref, int64_t S_total, int layout, int wire, const double* phi,
                          const double* expected, double mixture, const double* mix_host, double* phi_out, double* expected_out, uint8_t* path_out,
                          int64_t* n_calls)
{
  if (!m || !test || !ref || S_total <= 0) return ed_fail(ED_ERR_INVALID, "ed_multi_run_host: bad arguments");
  const int64_t D = (int64_t)m->devs.size(), n_slabs = (S_total + m->slab - 1) / m->slab;
  m->S_total = S_total;
  m->calls.clear(); m->info.clear();
  std::atomic<int64_t> queue{0};
  for (auto& d : m->devs) { d.segs.clear(); d.n_columns = 0; d.rc = ED_OK; d.err.clear(); d.seconds = 0.0; }
  auto work = [&](ed_multi::Dev* d, bool own_thread) {
    const auto t0 = std::chrono::steady_clock::now();
    try {
      if (own_thread && m->numa_bind) multi_bind_thread_to_node(d->numa_node);
      auto next = [&]() -> int64_t {
        const int64_t i = queue.fetch_add(1, std::memory_order_relaxed);
        if (i >= n_slabs) return -1;
        d->n_columns += std::min(m->slab, S_total - i * m->slab);
        return i;
      };
      int64_t k = 0;
      d->rc = cohort_run_host_slabs(d->cohort, test, ref, S_total, next, layout, wire, phi, expected, mixture, mix_host, phi_out, expected_out, path_out,
                                    &k, &d->segs);
    } catch (...) { d->rc = ed_caught("ed_multi_run_host"); }     // (nothing may leave a thread's function)
    if (d->rc != ED_OK) {
      queue.store(n_slabs, std::memory_order_relaxed);             // the others stop taking slabs: the run has failed
      try { d->err = g_last_error; } catch (...) {}                // (thread-local: carried to the caller's thread below)
    }
    d->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  if (D == 1) work(&m->devs[0], false);       // (the caller's thread: its affinity is the caller's business)
  else {
    ed_thread_pool pool;
    for (auto& d : m->devs) pool.start(work, &d, true);
    pool.join();
  }
  for (auto& d : m->devs)
    if (d.rc != ED_OK) {
      int64_t lo = -1, hi = -1;
      for (const auto& sg : d.segs) { lo = lo < 0 ? sg.slab : std::min(lo, sg.slab); hi = std::max(hi, sg.slab); }
      return ed_fail(d.rc, "device %d (columns %lld..%lld of its slabs): %s", d.device, (long long)(lo < 0 ? 0 : lo * m->slab),
                     (long long)(hi < 0 ? 0 : std::min(S_total, (hi + 1) * m->slab)), d.err.c_str());
    }
  // slab order = column order
  struct Src { const ed_multi::Dev* d; ed_slab_seg sg; };
  std::vector<Src> order;
  for (auto& d : m->devs) for (const auto& sg : d.segs) order.push_back({&d, sg});
  std::sort(order.begin(), order.end(), [](const Src& a, const Src& b) { return a.sg.slab < b.sg.slab; });
  for (const Src& o : order) {
    m->calls.insert(m->calls.end(), o.d->cohort->calls.begin() + o.sg.row0, o.d->cohort->calls.begin() + o.sg.row1);
    if (o.d->cohort->info.size() >= (size_t)o.sg.row1) m->info.insert(m->info.end(), o.d->cohort->info.begin() + o.sg.row0, o.d->cohort->info.begin() + o.sg.row1);
  }
  if (n_calls) *n_calls = (int64_t)m->calls.size();
  return ED_OK;
}

ED_EXPORT int ed_multi_run_host(ed_multi* m, const void* test, const void* ref, int64_t S_total, int layout, int wire, const double* phi,
                                const double* expected, double mixture, double* phi_out, double* expected_out, uint8_t* path_out, int64_t* n_calls)
try {
  return multi_run_host(m, test, ref, S_total, layout, wire, phi, expected, mixture, nullptr, phi_out, expected_out, path_out, n_calls);
}
ED_CATCH("ed_multi_run_host")

// every device's pipeline uploads the whole mixture vector once and its slabs take their windows of it (as for given phi / expected)
ED_EXPORT int ed_multi_run_host_mix(ed_multi* m, const void* test, const void* ref, int64_t S_total, int layout, int wire, const double* phi,
                                    const double* expected, const double* mixture, double* phi_out, double* expected_out, uint8_t* path_out,
                                    int64_t* n_calls)
try {
  if (!m || !test || !ref || S_total <= 0) return ed_fail(ED_ERR_INVALID, "ed_multi_run_host_mix: bad arguments");
  if (int rc = check_host_mixtures(mixture, S_total, "ed_multi_run_host_mix")) return rc;
  return multi_run_host(m, test, ref, S_total, layout, wire, phi, expected, 1.0, mixture, phi_out, expected_out, path_out, n_calls);
}
ED_CATCH("ed_multi_run_host_mix")

ED_EXPORT int ed_multi_copy_calls(ed_multi* m, ed_call* calls, ed_call_info* info, int64_t cap)
try {
  if (!m) return ed_fail(ED_ERR_INVALID, "NULL argument");
  const int64_t k = std::min<int64_t>(cap, (int64_t)m->calls.size());
  if (k > 0 && calls) std::memcpy(calls, m->calls.data(), (size_t)k * sizeof(ed_call));
  if (k > 0 && info && m->info.size() >= (size_t)k) std::memcpy(info, m->info.data(), (size_t)k * sizeof(ed_call_info));
  return ED_OK;
}
ED_CATCH("ed_multi_copy_calls")

ED_EXPORT int ed_multi_run_status(ed_multi* m, int64_t* n_unconverged, int64_t* n_gsl_errors)
try {
  if (!m) return ed_fail(ED_ERR_INVALID, "NULL argument");
  int64_t nu = 0, ne = 0;
  for (auto& d : m->devs) { nu += d.cohort->n_unconverged; ne += d.cohort->n_gsl_errors; }
  if (n_unconverged) *n_unconverged = nu;
  if (n_gsl_errors) *n_gsl_errors = ne;
  return ED_OK;
}
ED_CATCH("ed_multi_run_status")

ED_EXPORT int ed_multi_table_status(ed_multi* m, int64_t out[4])
try {
  if (!m || !out) return ed_fail(ED_ERR_INVALID, "NULL argument");
  for (int q = 0; q < 4; ++q) { out[q] = 0; for (auto& d : m->devs) out[q] += d.cohort->tab_stats[q]; }
  return ED_OK;
}
ED_CATCH("ed_multi_table_status")

// option phi_bins > 1: phi.estimates [phi_bins][S_total], complete.bins [(phi_bins + 1)][S_total] of the last run (every device wrote the columns of its slabs)
ED_EXPORT int ed_multi_copy_bins(ed_multi* m, double* phi_bins_out, double* edges_out)
try {
  if (!m) return ed_fail(ED_ERR_INVALID, "NULL argument");
  const int B = m->phi_bins;
  if (B < 2) return ed_fail(ED_ERR_STATE, "ed_multi_copy_bins: no depth-binned run to report");
  const int64_t S = m->S_total;
  for (auto& d : m->devs) {
    if (d.segs.empty()) continue;
    if (d.cohort->h_phib.size() != (size_t)B * S) return ed_fail(ED_ERR_STATE, "ed_multi_copy_bins: no depth-binned run to report");
    for (const auto& sg : d.segs) {
      const int64_t s0 = sg.slab * m->slab, n = std::min(m->slab, S - s0);
      for (int g = 0; g < B; ++g) if (phi_bins_out) std::memcpy(phi_bins_out + (size_t)g * S + s0, &d.cohort->h_phib[(size_t)g * S + s0], (size_t)n * 8);
      for (int g = 0; g <= B; ++g) if (edges_out) std::memcpy(edges_out + (size_t)g * S + s0, &d.cohort->h_edges[(size_t)g * S + s0], (size_t)n * 8);
    }
  }
  return ED_OK;
}
ED_CATCH("ed_multi_copy_bins")

// what every device did in the last run: slabs and columns it took from the queue, wall seconds of its thread, the NUMA node its thread was kept on
// (-1: unknown or not bound).  Arrays of ed_multi_n_devices entries; any may be NULL.  An uneven split is the queue at work (or a device in trouble).
ED_EXPORT int ed_multi_device_stats(ed_multi* m, int* devices, int64_t* n_slabs, int64_t* n_columns, double* seconds, int* numa_nodes)
try {
  if (!m) return ed_fail(ED_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < m->devs.size(); ++i) {
    if (devices) devices[i] = m->devs[i].device;
    if (n_slabs) n_slabs[i] = (int64_t)m->devs[i].segs.size();
    if (n_columns) n_columns[i] = m->devs[i].n_columns;
    if (seconds) seconds[i] = m->devs[i].seconds;
    if (numa_nodes) numa_nodes[i] = m->devs[i].numa_node;
  }
  return ED_OK;
}
ED_CATCH("ed_multi_device_stats")
