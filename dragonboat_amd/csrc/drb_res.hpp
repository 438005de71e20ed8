// drb_res.hpp -- the owners of the engine's device resources, included by
// drb_engine.hip only.  Two concepts, a buffer (Buf) and a handle (Handle):
// move-only, empty by default, releasing what they hold when they go.  A
// struct of them needs no hand-kept free list, and one built behind a
// std::unique_ptr and abandoned half way leaves nothing behind.
//
// Plain C++17, the allocator and the destroy call template parameters
// (tests/native/res_owner.cpp runs the types on a counting fake under
// AddressSanitizer); the HIP and HSA backends below need a HIP compile.
#pragma once

#include <stddef.h>

#include <utility>

namespace drb {

// One allocation of A (`static int alloc(void **, size_t)`, 0 on success,
// and `static void free(void *)`): {p, cap} is a live allocation of cap
// bytes or {nullptr, 0}, after a failure too.
template <class A>
struct Buf {
  void *p = nullptr;
  size_t cap = 0;

  Buf() = default;
  Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~Buf() { reset(); }

  void reset() {
    if (p) A::free(p);
    p = nullptr, cap = 0;
  }
  // grow-only, the contents are not kept; any rounding is the caller's
  int reserve(size_t need) { return need <= cap ? 0 : grow(need); }
  template <class T>
  T *as() const {
    return static_cast<T *>(p);
  }

 private:
  int grow(size_t need) {
    reset();
    const int rc = A::alloc(&p, need);
    if (rc)
      p = nullptr;
    else
      cap = need;
    return rc;
  }
};

// One runtime handle (a stream, an event, an HSA signal); D supplies `static
// bool null(T)` and `static void destroy(T)`.  Converts to the raw handle,
// so launch sites read as before.
template <class T, class D>
struct Handle {
  T h{};

  Handle() = default;
  Handle(Handle &&o) noexcept : h(o.h) { o.h = T{}; }
  Handle &operator=(Handle &&o) noexcept {
    if (this != &o) {
      reset();
      std::swap(h, o.h);
    }
    return *this;
  }
  ~Handle() { reset(); }

  void reset() {
    if (!D::null(h)) D::destroy(h);
    h = T{};
  }
  operator T() const { return h; }
  explicit operator bool() const { return !D::null(h); }
  T *out() {  // for a create call: what it held goes first
    reset();
    return &h;
  }
};

}  // namespace drb

#ifdef __HIPCC__
namespace drb {

// hipFree, not hipFreeAsync: growth paths free a buffer that work already
// enqueued on an engine stream may still read (scratch() is the clearest
// case) and rely on hipFree's implicit device wait.  The explicit stream
// waits at some growth sites (worker_reserve, the staging upload) order host
// threads and copy engines as well, and stay.
static inline int hip_alloc_rc(hipError_t r, const char *what, size_t bytes) {
  if (r != hipSuccess)
    fprintf(stderr, "drb_engine: %s of %zu bytes failed: %s\n", what, bytes,
            hipGetErrorString(r));
  return r != hipSuccess;
}
struct HipDevice {
  static int alloc(void **p, size_t n) {
    return hip_alloc_rc(hipMalloc(p, n), "hipMalloc", n);
  }
  static void free(void *p) { (void)hipFree(p); }
};
template <unsigned Flags>
struct HipPinned {
  static int alloc(void **p, size_t n) {
    return hip_alloc_rc(hipHostMalloc(p, n, Flags), "hipHostMalloc", n);
  }
  static void free(void *p) { (void)hipHostFree(p); }
};
using DevBuf = Buf<HipDevice>;
template <unsigned Flags>
using PinnedBuf = Buf<HipPinned<Flags>>;

// (a failed create leaves the handle empty)
struct StreamDestroy {
  static bool null(hipStream_t s) { return !s; }
  static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct Stream : Handle<hipStream_t, StreamDestroy> {
  hipError_t create() {
    const hipError_t r = hipStreamCreateWithFlags(out(), hipStreamNonBlocking);
    if (r != hipSuccess) h = nullptr;
    return r;
  }
};
struct EventDestroy {
  static bool null(hipEvent_t e) { return !e; }
  static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct Event : Handle<hipEvent_t, EventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    const hipError_t r = hipEventCreateWithFlags(out(), flags);
    if (r != hipSuccess) h = nullptr;
    return r;
  }
};
struct SignalDestroy {  // (hsa_signal_t: after drb_hsa.hpp)
  static bool null(hsa_signal_t s) { return !s.handle; }
  static void destroy(hsa_signal_t s) { (void)hsa_signal_destroy(s); }
};
struct Signal : Handle<hsa_signal_t, SignalDestroy> {
  hsa_status_t create() {
    const hsa_status_t r = hsa_signal_create(0, 0, nullptr, out());
    if (r != HSA_STATUS_SUCCESS) h = hsa_signal_t{0};
    return r;
  }
};

}  // namespace drb
#endif  // __HIPCC__
