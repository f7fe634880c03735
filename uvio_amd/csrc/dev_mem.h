// Scoped owners of device memory, pinned host memory, streams and events.  Move-only; each converts implicitly
// to the raw handle it owns, so call sites read as they would with a plain pointer.  Destructors ignore the
// HIP return code and never throw.
#pragma once
#include <algorithm>
#include <utility>

#include "hp_common.h"

namespace uvhp {

// n elements of T (at least one) in device (hipMalloc) or pinned host (hipHostMalloc) memory
template <class T, bool Pinned>
class MemBuf {
 public:
  MemBuf() = default;
  explicit MemBuf(size_t n) {
    n = std::max<size_t>(n, 1);
    void *p = nullptr;
    if (Pinned)
      HP_HIP(hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault));
    else
      HP_HIP(hipMalloc(&p, n * sizeof(T)));
    p_ = (T *)p;
    n_ = n;
  }
  MemBuf(MemBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  MemBuf &operator=(MemBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  ~MemBuf() { reset(); }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  size_t size() const { return n_; }  // elements
  operator T *() const & { return p_; }
  operator T *() const && = delete;  // a temporary's memory is gone before the pointer could be used

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};
template <class T>
using DevBuf = MemBuf<T, false>;
template <class T>
using PinBuf = MemBuf<T, true>;

// a stream (hipStreamNonBlocking) or an event (hipEventDisableTiming); default-constructed: empty
template <class H, hipError_t (*Destroy)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  HipHandle &operator=(HipHandle &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~HipHandle() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};
struct Stream : HipHandle<hipStream_t, hipStreamDestroy> {
  static Stream create() {
    Stream s;
    HP_HIP(hipStreamCreateWithFlags(&s.h_, hipStreamNonBlocking));
    return s;
  }
};
struct Event : HipHandle<hipEvent_t, hipEventDestroy> {
  static Event create() {
    Event e;
    HP_HIP(hipEventCreateWithFlags(&e.h_, hipEventDisableTiming));
    return e;
  }
};

}  // namespace uvhp
