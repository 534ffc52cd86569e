// A stand-in for <hip/hip_runtime.h> on the CPU, only what hg_dev.h uses:
// allocations over malloc, streams and events as counted tokens, a switch that
// fails the next allocation, and live counts per kind
// (tests/native/dev_owners_host.cpp).
#pragma once
#include <cstddef>
#include <cstdlib>

typedef enum { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;
enum { hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0 };

namespace fakehip {
struct Counts {
  long dev = 0, host = 0, streams = 0, events = 0;  // live handles
  long dev_frees = 0;                               // hipFree calls on a live block
  size_t last_dev_bytes = 0;
  unsigned last_event_flags = 0;
  bool fail_next_alloc = false;
};
inline Counts& counts() {
  static Counts c;
  return c;
}
inline hipError_t allocate(void** p, size_t bytes, long& live) {
  if (counts().fail_next_alloc) {
    counts().fail_next_alloc = false;
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  live++;
  return hipSuccess;
}
}  // namespace fakehip

template <typename T>
inline hipError_t hipMalloc(T** p, size_t bytes) {
  fakehip::counts().last_dev_bytes = bytes;
  return fakehip::allocate(reinterpret_cast<void**>(p), bytes, fakehip::counts().dev);
}
inline hipError_t hipFree(void* p) {
  if (p) {
    fakehip::counts().dev--;
    fakehip::counts().dev_frees++;
  }
  free(p);
  return hipSuccess;
}
template <typename T>
inline hipError_t hipHostMalloc(T** p, size_t bytes, unsigned) {
  return fakehip::allocate(reinterpret_cast<void**>(p), bytes, fakehip::counts().host);
}
inline hipError_t hipHostFree(void* p) {
  if (p) fakehip::counts().host--;
  free(p);
  return hipSuccess;
}
// tokens are heap blocks, so the sanitizer reports one destroyed twice or never
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = static_cast<hipStream_t>(malloc(1));
  fakehip::counts().streams++;
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  fakehip::counts().streams--;
  free(s);
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  *e = static_cast<hipEvent_t>(malloc(1));
  fakehip::counts().events++;
  fakehip::counts().last_event_flags = flags;
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  fakehip::counts().events--;
  free(e);
  return hipSuccess;
}
