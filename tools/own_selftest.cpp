// The owners of csrc/ed_own.hpp on their own: a stand-alone program (its own main, no library, no Python) for a sanitizer build of the
// HOST code:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize
//         -Iexomedepth_amd/csrc -o own_selftest tools/own_selftest.cpp
// It runs with or without a device.  Without one every allocation fails, and what is checked is that a failure leaves the owner empty and the
// counters untouched; with one the same statements check that the counters follow the allocations.  Either way: moves transfer and empty
// their source, reset() of an empty owner does nothing, and a set of buffers built into a local is released whole when the local goes.
// Exit status 0 and "own_selftest ok".
#include <cstdio>
#include <utility>
#include <vector>

#include "ed_own.hpp"

using namespace edown;

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "own_selftest: line %d: %s\n", __LINE__, #x); ++g_failed; } } while (0)

static int64_t live_n() { return g_live_n.load(); }
static int64_t live_bytes() { return g_live_bytes.load(); }

struct Set { DevBuf<double> a; DevBuf<int> b; PinBuf<char> c; };

// as the library builds its lazily made sets: into a local, moved out on success only.  fail_at: pretend allocation number fail_at failed
static bool build_set(Set& out, int fail_at)
{
  Set t;
  bool ok = true;
  int k = 0;
  auto A = [&](auto& buf, size_t bytes) { if (ok && (k++ == fail_at || buf.alloc(bytes) != hipSuccess)) ok = false; };
  A(t.a, 800); A(t.b, 400); A(t.c, 64);
  if (!ok) { (void)hipGetLastError(); return false; }
  out = std::move(t);
  return true;
}

int main()
{
  CHECK(live_n() == 0 && live_bytes() == 0);
  {
    DevBuf<double> a;
    CHECK(!a && a.get() == nullptr && a.bytes() == 0);
    a.reset();                                            // empty: harmless
    CHECK(live_n() == 0 && live_bytes() == 0);
    const bool have = a.alloc(0) == hipSuccess;           // 0 bytes: one byte, as the library always allocated
    if (!have) (void)hipGetLastError();
    std::printf("own_selftest: device memory %s\n", have ? "available" : "not available (every allocation fails)");
    CHECK((bool)a == have && a.bytes() == (have ? 1u : 0u));
    CHECK(live_n() == (have ? 1 : 0) && live_bytes() == (have ? 1 : 0));
    CHECK((a.alloc(4096) == hipSuccess) == have);         // what was held goes first
    CHECK((bool)a == have && live_n() == (have ? 1 : 0) && live_bytes() == (have ? 4096 : 0));
    double* const p = a.get();
    DevBuf<double> b(std::move(a));                       // move construction
    CHECK(!a && a.bytes() == 0 && b.get() == p && b.bytes() == (have ? 4096u : 0u));
    DevBuf<double> c;
    CHECK((c.alloc(64) == hipSuccess) == have);
    c = std::move(b);                                     // move assignment: c's own block is released, b's taken over
    CHECK(!b && c.get() == p && live_n() == (have ? 1 : 0) && live_bytes() == (have ? 4096 : 0));
    DevBuf<double>& same = c;
    c = std::move(same);                                  // self-assignment keeps it
    CHECK(c.get() == p);
    CHECK(c.reserve(100) == hipSuccess || !have);         // grow-only: large enough, kept
    CHECK(c.get() == p);
    CHECK((c.reserve(8192) == hipSuccess) == have);       // too small: a fresh block
    CHECK(c.bytes() == (have ? 8192u : 0u) && live_bytes() == (have ? 8192 : 0));
    PinBuf<int> h;
    const bool have_pin = h.alloc(4) == hipSuccess;
    if (!have_pin) (void)hipGetLastError();
    CHECK((bool)h == have_pin && live_n() == (have ? 1 : 0) + (have_pin ? 1 : 0));
    if (have_pin) { *h = -1; CHECK(h[0] == -1); }
    std::vector<DevBuf<void>> v;                          // in a container that reallocates
    for (int i = 0; i < 9; ++i) { v.emplace_back(); (void)v.back().reserve(16); }
    CHECK(live_n() == (have ? 10 : 0) + (have_pin ? 1 : 0));
  }
  CHECK(live_n() == 0 && live_bytes() == 0);              // everything above went with its scope
  (void)hipGetLastError();
  for (int fail_at = 0; fail_at <= 3; ++fail_at) {        // a set that fails half-way leaves nothing; fail_at = 3: none fails on purpose
    Set s;
    const bool made = build_set(s, fail_at);
    CHECK(made ? (s.a && s.b && s.c && live_n() == 3 && live_bytes() == 1264) : (!s.a && !s.b && !s.c && live_n() == 0 && live_bytes() == 0));
    CHECK(fail_at == 3 || !made);
  }
  CHECK(live_n() == 0 && live_bytes() == 0);
  {
    Event e, f;
    e.reset();
    const bool have_ev = e.create(hipEventDisableTiming) == hipSuccess;
    if (!have_ev) (void)hipGetLastError();
    CHECK((bool)e == have_ev);
    const hipEvent_t raw = e.get();
    f = std::move(e);
    CHECK(!e && f.get() == raw);
    Event g(std::move(f));
    CHECK(!f && g.get() == raw);
    EventSet<3> set;                                      // made on first use, kept from then on; live is the user's to set, drop() clears it
    CHECK(!set.live && !set.ev[0] && !set.ev[2]);
    const bool have_set = set.ready() == hipSuccess;
    if (!have_set) (void)hipGetLastError();
    CHECK(have_set == have_ev && (bool)set.ev[0] == have_set && (bool)set.ev[2] == have_set && !set.live);
    const hipEvent_t first = set.ev[0].get();
    CHECK((set.ready() == hipSuccess) == have_set && set.ev[0].get() == first);      // a second call makes nothing new
    if (have_set) {
      float ms = -1.f;
      CHECK(set.record(0, nullptr) == hipSuccess && set.record(2, nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess);
      CHECK(set.elapsed(0, 2, &ms) == hipSuccess && ms >= 0.f);
    }
    set.live = true;
    set.drop();
    CHECK(!set.live && set.ev[0].get() == first);         // the events stay
    Stream s, t;
    s.reset();
    CHECK(!s && s.get() == nullptr);
    hipStream_t made = nullptr;
    if (hipStreamCreateWithFlags(&made, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); made = nullptr; }
    s.reset(made);
    t = std::move(s);
    CHECK(!s && t.get() == made);
    Stream u(std::move(t));
    CHECK(!t && u.get() == made);
  }
  if (g_failed) { std::fprintf(stderr, "own_selftest: %d checks failed\n", g_failed); return 1; }
  std::printf("own_selftest ok\n");
  return 0;
}
