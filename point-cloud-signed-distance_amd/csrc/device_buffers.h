// device_buffers.h — owners of the context's HIP resources: grow-only device
// and pinned host buffers, streams and events. Header-only, move-only, no
// exceptions (errors come back as hipError_t), no allocator behind them.
//
// The rule for their users: a raw pointer leaves a buffer only through get(),
// after the reserve() for that use. Nothing keeps a raw copy across a call that
// may reserve — a reserve that grows frees the old allocation, and a pointer
// taken before it would hand a launch freed (or not yet allocated) memory. The
// structs that kernels take by value (LocalModel, PosedModel, PassOutputs, ...)
// are such copies: non-owning views, filled right after the reserves they show.
//
// Nothing here synchronises. Where queued work may still read a buffer, the
// caller synchronises the stream before the reserve that replaces it. Every
// free goes to the current device: set the context's device first.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

// (internal types: they and their instantiations stay out of the library's exports)
#pragma GCC visibility push(hidden)
namespace fsdf {

struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

// A pointer and its capacity in elements of T (buffers whose element type
// follows the context precision are Buf<unsigned char>, in bytes).
template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  Buf& operator=(Buf&& o) noexcept {
    Buf(std::move(o)).swap(*this);  // (the old allocation leaves with the temporary)
    return *this;
  }
  ~Buf() { reset(); }

  // Room for n elements: kept when there already is, else freed and allocated
  // anew at exactly n (no growth factor; one element for n = 0, so the pointer
  // is never null after a reserve). The contents do not survive a reallocation.
  hipError_t reserve(size_t n) {
    if (cap_ >= n && p_) return hipSuccess;
    reset();
    if (n == 0) n = 1;
    const hipError_t e = Mem::alloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else cap_ = n;
    return e;
  }
  void reset() {
    if (p_) Mem::release((void*)p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  void swap(Buf& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <typename T, typename Mem>
void swap(Buf<T, Mem>& a, Buf<T, Mem>& b) noexcept {
  a.swap(b);
}
template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinnedBuf = Buf<T, PinnedMem>;

// A non-blocking stream / an event, destroyed with their owner. They convert
// to the runtime's handle (null until create()).
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace fsdf
#pragma GCC visibility pop
