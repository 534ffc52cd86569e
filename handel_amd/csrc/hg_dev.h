// hg_dev.h — move-only owners of the HIP handles the host code keeps: device
// buffers, streams, events and pinned host allocations. Plain host C++ over
// the HIP runtime API. A struct of these frees what it holds when it is
// destroyed; nothing else in the host code frees or destroys a handle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace hg {

// A device allocation of `cap` elements. ensure() only grows (at least 64
// elements; the old block is freed before the new one is allocated); on
// failure the buffer is empty.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  // exactly n elements (the fixed-size tables: no floor)
  hipError_t alloc(size_t n) {
    reset();
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  hipError_t ensure(size_t n) { return n <= cap ? hipSuccess : alloc(n < 64 ? 64 : n); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  size_t bytes() const { return cap * sizeof(T); }
};

// One handle of the runtime, destroyed with Destroy; converts to the raw handle.
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return hipStreamCreateWithFlags(&h, flags);
  }
};

// flags: hipEventDefault (timing) or hipEventDisableTiming (ordering only)
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return hipEventCreateWithFlags(&h, flags);
  }
};

// pinned host memory of n elements
template <typename T>
struct HostBuf : Handle<void*, hipHostFree> {
  hipError_t alloc(size_t n) {
    reset();
    return hipHostMalloc(&h, n * sizeof(T), hipHostMallocDefault);
  }
  T* get() const { return static_cast<T*>(h); }
};

}  // namespace hg
