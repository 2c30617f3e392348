// ed_own.hpp -- move-only owners of what libedcore obtains from the HIP runtime: device memory, pinned host memory, events and
// streams.  Host-only types.  Every byte of device or pinned memory the library owns is obtained and released here and nowhere
// else, which is what makes the two counters below exact (ed_live_allocations).  Memory handed out by ed_malloc / ed_host_alloc
// belongs to the caller and does not pass through here.
//
// Nothing here synchronises: a site that has to wait for a stream before a buffer or the stream itself goes says so itself.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace edown {

inline std::atomic<int64_t> g_live_n{0}, g_live_bytes{0};   // library-owned allocations alive / their bytes

// kPinned = false: device memory (hipMalloc); true: pinned host memory (hipHostMalloc, default flags)
template <class T, bool kPinned>
class Buf {
  T* p_ = nullptr;
  size_t bytes_ = 0;

public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  Buf& operator=(Buf&& o) noexcept
  {
    if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  ~Buf() { reset(); }

  // a fresh allocation of `bytes` (at least one); what was held goes first.  On failure the owner is empty and the runtime's
  // error is returned, still pending for hipGetLastError
  hipError_t alloc(size_t bytes)
  {
    reset();
    const size_t n = bytes ? bytes : 1;
    void* q = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&q, n, hipHostMallocDefault) : hipMalloc(&q, n);
    if (e != hipSuccess) return e;
    p_ = (T*)q; bytes_ = n;
    g_live_n.fetch_add(1, std::memory_order_relaxed);
    g_live_bytes.fetch_add((int64_t)n, std::memory_order_relaxed);
    return hipSuccess;
  }
  // grow-only use: keeps what it holds if that is large enough, else frees it and allocates anew (nothing is copied)
  hipError_t reserve(size_t bytes) { return (p_ && bytes_ >= bytes) ? hipSuccess : alloc(bytes); }
  void reset()
  {
    if (!p_) return;
    (void)(kPinned ? hipHostFree((void*)p_) : hipFree((void*)p_));
    g_live_n.fetch_sub(1, std::memory_order_relaxed);
    g_live_bytes.fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
    p_ = nullptr; bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  template <class U> U* as() const { return (U*)p_; }
  explicit operator bool() const { return p_ != nullptr; }
  size_t bytes() const { return bytes_; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

class Event {
  hipEvent_t e_ = nullptr;

public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~Event() { reset(); }
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&e_, flags); }
  void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
  hipEvent_t get() const { return e_; }
  operator hipEvent_t() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }
};

// N events made on first use, and whether they hold something: `live` is set by whoever recorded all of them and cleared (drop) by
// whatever makes their times stale.  The events themselves are kept from one use to the next.
template <int N>
struct EventSet {
  Event ev[N];
  bool live = false;
  hipError_t ready()
  {
    hipError_t rc = hipSuccess;
    for (auto& e : ev) { if (!e && rc == hipSuccess) rc = e.create(); }
    return rc;
  }
  hipError_t record(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
  hipError_t elapsed(int i, int j, float* ms) const { return hipEventElapsedTime(ms, ev[i], ev[j]); }
  void drop() { live = false; }
};

// destroys without synchronising (the runtime lets queued work finish)
class Stream {
  hipStream_t s_ = nullptr;

public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
  ~Stream() { reset(); }
  void reset(hipStream_t adopt = nullptr) { if (s_) (void)hipStreamDestroy(s_); s_ = adopt; }   // takes over a stream made elsewhere
  hipStream_t get() const { return s_; }
  operator hipStream_t() const { return s_; }
  explicit operator bool() const { return s_ != nullptr; }
};

}  // namespace edown
