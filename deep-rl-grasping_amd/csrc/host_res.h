// host_res.h -- owners of what a handle holds outside the caller's arenas: page-locked host blocks, events, the side stream and
// the ring of two staging buffers.  Host code only, nothing virtual, everything inline; included by engine.hip in front of
// grl_ctx (after the HIP runtime header or its emulation).  None is copyable; each releases what it holds in its destructor.
#pragma once
#include <cstring>

// One hipHostMalloc block of T.
template <class T>
class Pinned {
  T* p_ = nullptr;
  size_t n_ = 0;
 public:
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { reset(); }
  // Only grows: frees the old block and allocates a new, zeroed one.  Content is NOT kept and nothing is synchronised -- the
  // caller's contract is that the previous call has finished with the block (the entry points that stage through one
  // synchronise the stream, or wait for their completion counter, before they return).
  hipError_t reserve(size_t n, unsigned flags = 0) {
    if (n <= n_) return hipSuccess;
    reset();
    const hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), flags);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    memset(p_, 0, n * sizeof(T));
    n_ = n;
    return hipSuccess;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
};

// A hipEvent_t created on first use, with the flags given then (0: a timing event, as hipEventCreate makes).
class Event {
  hipEvent_t e_ = nullptr;
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }    // (a std::vector<Event> grows; with it the copies are gone)
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create(unsigned flags = hipEventDisableTiming) {      // (no-op once it exists)
    const hipError_t e = e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) e_ = nullptr;
    return e;
  }
  hipEvent_t raw() const { return e_; }
};

// A non-blocking stream created on first use (the second capture lane).
class Stream {
  hipStream_t s_ = nullptr;
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  hipError_t get(hipStream_t* out) {
    const hipError_t e = s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e != hipSuccess) s_ = nullptr;
    *out = s_;
    return e;
  }
};

// Two page-locked buffers used in turn, each guarded by an event, so the host never waits for the GPU unless it is two calls
// ahead: acquire() hands out the current slot once the work recorded at its last release has finished; the caller fills it and
// enqueues what reads it; release(stream) records the slot's event behind that work and flips the ring.  A call that fails
// between the two keeps the slot for the next one.  Both slots are allocated (zeroed) at the first acquire: n is a constant of the handle.
template <class T>
class StagingRing {
  Pinned<T> buf_[2];
  Event ev_[2];
  bool used_[2] = {false, false};      // the slot's event has been recorded
  int next_ = 0;
 public:
  hipError_t acquire(size_t n, T** out) {
    hipError_t e = buf_[0].reserve(n);
    if (e == hipSuccess) e = buf_[1].reserve(n);
    if (e == hipSuccess && used_[next_]) e = hipEventSynchronize(ev_[next_].raw());
    if (e == hipSuccess) *out = buf_[next_].get();
    return e;
  }
  hipError_t release(hipStream_t stream) {
    hipError_t e = ev_[next_].create();
    if (e == hipSuccess) e = hipEventRecord(ev_[next_].raw(), stream);
    if (e == hipSuccess) { used_[next_] = true; next_ ^= 1; }
    return e;
  }
};
