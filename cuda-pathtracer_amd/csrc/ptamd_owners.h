// ptamd_owners.h — who frees what on the host side of libptamd.so: a device buffer, a pinned host buffer, an event and a stream,
// each a move-only handle that releases in its destructor (the release's error is ignored: there is no one to report it to) and is
// empty after a move.  Structs that hold them are move-only too, and nothing else in the host API calls a release function.
// Kernel parameter structs keep raw pointers, filled from get().
#pragma once

#include <hip/hip_runtime.h>

namespace ptamd {

template <typename T>
class DeviceBuffer {
public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~DeviceBuffer() { reset(); }
  // frees what it holds first (hipFree waits for the work in flight that may still use it); empty when the allocation fails
  hipError_t alloc(size_t bytes)
  {
    reset();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), bytes);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
private:
  T* p_ = nullptr;
};

template <typename T>
class PinnedBuffer {
public:
  PinnedBuffer() = default;
  PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~PinnedBuffer() { reset(); }
  hipError_t alloc(size_t bytes)
  {
    reset();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), bytes, hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
private:
  T* p_ = nullptr;
};

// An event without timing, created at its first use
class Event {
public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~Event() { reset(); }
  hipError_t ensure() { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, hipEventDisableTiming); }
  void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
  hipEvent_t get() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }
private:
  hipEvent_t e_ = nullptr;
};

class Stream {
public:
  Stream() = default;
  explicit Stream(hipStream_t made) : s_(made) {}   // takes over a stream its caller has just created
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
  ~Stream() { reset(); }
  hipError_t create_non_blocking()
  {
    reset();
    const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e != hipSuccess) s_ = nullptr;
    return e;
  }
  void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
  hipStream_t get() const { return s_; }
  explicit operator bool() const { return s_ != nullptr; }
private:
  hipStream_t s_ = nullptr;
};

} // namespace ptamd
