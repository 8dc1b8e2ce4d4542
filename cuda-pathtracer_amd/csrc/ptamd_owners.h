// ptamd_owners.h — who frees what on the host side of libptamd.so: a device buffer, a pinned host buffer, an event and a stream,
// each a move-only handle that releases in its destructor (the release's error is ignored: there is no one to report it to) and is
// empty after a move.  Structs that hold them are move-only too, and nothing else in the host API calls a release function.
// Kernel parameter structs keep raw pointers, filled from get().  Behind the owners: the two staging types built on them.
#pragma once

#include <hip/hip_runtime.h>

#include "ptamd_tuning.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ptamd {

// Under PTAMD_ALLOC_FILL (ptamd_tuning.h): every byte of a new allocation set to `byte`, on the device before this returns (the
// fill goes to the null stream, which the context's own streams do not wait for: hence the device-wide wait)
inline hipError_t fill_new(void* p, int byte, size_t bytes, bool pinned)
{
  if (pinned) { std::memset(p, byte, bytes); return hipSuccess; }
  const hipError_t e = hipMemset(p, byte, bytes);
  return e != hipSuccess ? e : hipDeviceSynchronize();
}

// One allocation of T's: device memory (hipMalloc / hipFree) or pinned host memory (hipHostMalloc / hipHostFree)
template <typename T, bool Pinned>
class Buffer {
public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Buffer& operator=(Buffer&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~Buffer() { reset(); }
  // frees what it holds first (hipFree waits for the work in flight that may still use it); empty when the allocation fails
  hipError_t alloc(size_t bytes)
  {
    reset();
    void** p = reinterpret_cast<void**>(&p_);
    const hipError_t e = Pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    const int fill = alloc_fill_byte();   // tuning knob PTAMD_ALLOC_FILL; off (-1): no call beyond the allocation
    return fill < 0 ? hipSuccess : fill_new(p_, fill, bytes, Pinned);
  }
  void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
private:
  T* p_ = nullptr;
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

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

// ---- "Two pinned slots used in turn", once for each direction.  The host may run two calls ahead of the device: it fills (or reads)
// one slot while the copy out of (or into) the other may still be in flight, and a copy that lands late never touches the words of a
// newer call.  Both types allocate at the first call that needs them: a scene that is never updated owns no pinned memory and no events.

// Host to device.  The device destination stays with the caller.
template <typename T>
class Upload {
public:
  hipError_t ensure(size_t bytes)   // at the first use: two slots of `bytes` bytes, their events
  {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i)
      if ((e = h_[i] ? hipSuccess : h_[i].alloc(bytes)) == hipSuccess) e = sent_[i].ensure();
    return e;
  }
  // the slot whose last copy is two calls back, once that copy has finished: the host may fill host(*slot)
  hipError_t acquire(uint32_t* slot)
  {
    *slot = next_++ & 1u;
    return valid_[*slot] ? hipEventSynchronize(sent_[*slot].get()) : hipSuccess;
  }
  T* host(uint32_t slot) const { return h_[slot].get(); }
  hipError_t sent(uint32_t slot, hipStream_t stream)   // behind the copies out of the slot that the caller has enqueued on `stream`
  {
    const hipError_t e = hipEventRecord(sent_[slot].get(), stream);
    if (e == hipSuccess) valid_[slot] = true;
    return e;
  }
  hipError_t drain() const   // the host waits for the copies out of both slots: the slots may then be replaced by larger ones
  {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) if (valid_[i]) e = hipEventSynchronize(sent_[i].get());
    return e;
  }
private:
  PinnedBuffer<T> h_[2];
  Event sent_[2];                          // the copy out of h_[i] has finished
  bool valid_[2] = { false, false };
  uint32_t next_ = 0;
};

// Device to host: a few words copied back behind the kernels that form them, read by the host only when someone asks.
template <typename T>
class ReadBack {
public:
  hipError_t ensure(uint32_t words)   // at the first use: one pinned buffer of two slots of `words` words, their events
  {
    words_ = words;
    hipError_t e = h_ ? hipSuccess : h_.alloc(2u * (size_t)words * sizeof(T));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = ready_[i].ensure();
    return e;
  }
  bool pending() const { return pending_; }
  // `stream` waits for the copies of earlier calls: they read the device words the caller is about to overwrite, possibly on
  // another stream
  hipError_t wait_on(hipStream_t stream) const
  {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) if (valid_[i]) e = hipStreamWaitEvent(stream, ready_[i].get(), 0);
    return e;
  }
  hipError_t enqueue(const T* src, hipStream_t stream)   // the copy of src's words into the next slot, its event behind it; pending
  {
    const uint32_t slot = next_++ & 1u;
    hipError_t e = hipMemcpyAsync(h_.get() + (size_t)slot * words_, src, words_ * sizeof(T), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess || (e = hipEventRecord(ready_[slot].get(), stream)) != hipSuccess) return e;
    valid_[slot] = pending_ = true;
    slot_ = slot;
    return hipSuccess;
  }
  hipError_t settle(const T** words)   // the host waits for the last copy enqueued; *words: what it brought
  {
    const hipError_t e = hipEventSynchronize(ready_[slot_].get());
    if (e != hipSuccess) return e;
    *words = h_.get() + (size_t)slot_ * words_;
    pending_ = false;
    return hipSuccess;
  }
  void supersede() { pending_ = false; }   // newer values are here by another way: what is pending is never waited for
  hipError_t drain() const   // the host waits for the copies into both slots
  {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) if (valid_[i]) e = hipEventSynchronize(ready_[i].get());
    return e;
  }
private:
  PinnedBuffer<T> h_;
  Event ready_[2];                         // the copy into slot i has finished
  bool valid_[2] = { false, false };
  uint32_t words_ = 0, next_ = 0, slot_ = 0;
  bool pending_ = false;
};

} // namespace ptamd
