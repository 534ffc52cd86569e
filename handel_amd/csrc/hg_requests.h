// hg_requests.h — what an aggregate request (hg_request) must satisfy, stated
// once for the host files and the kernels: the level rule of the reference and
// the bound of a request's bitset words, and the host's one walk over a batch.
// Plain C++ over include/handel_gpu.h (no HIP header): tests/native/
// requests_host.cpp compiles it with the host compiler alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/handel_gpu.h"

// host and device under the device compiler, nothing under a host compiler
#if defined(__HIPCC__)
#define HG_HOST_DEV __host__ __device__ __forceinline__
#else
#define HG_HOST_DEV inline
#endif

namespace hg {

// processing.go:350-352: the bitset has the level's size and lies in the registry
HG_HOST_DEV bool level_ok(const hg_request& r, uint64_t nreg) {
  return r.bitlen == r.level_size && (uint64_t)r.offset + r.bitlen <= nreg;
}
// the request's ceil(bitlen / 64) bitset words lie inside the batch's nwords
// (64-bit throughout: no request value wraps it)
HG_HOST_DEV bool words_ok(const hg_request& r, uint64_t nwords) {
  return (uint64_t)r.word_offset + ((uint64_t)r.bitlen + 63) / 64 <= nwords;
}

// Which requests of a batch must keep their words inside the bitset. The host
// entry points (hg_verify_aggregate*, hg_aggregate_pk, hg_verify_multisig*)
// skip a request that fails the level rule: its code is HG_ERR_LEVEL and no
// kernel reads its words. hg_lane_submit checks every request.
enum class WordsRule { kSkipLevelErrors, kEveryRequest };
static constexpr size_t kNoRequest = ~(size_t)0;
struct NoVisit {
  void operator()(const hg_request&) const {}
};

// One walk over a batch: the index of the first request the rule holds to the
// bitset whose words leave it, or kNoRequest. lvl (nullable): HG_OK or
// HG_ERR_LEVEL per request, filled up to where the walk stopped. visit(r) runs
// for every request that was checked and passed (the fold's capacities).
template <class Visit = NoVisit>
inline size_t first_request_outside(const hg_request* reqs, size_t n, uint64_t nreg, uint64_t nwords, WordsRule rule,
                                    int32_t* lvl = nullptr, Visit visit = Visit()) {
  for (size_t i = 0; i < n; i++) {
    const bool ok = level_ok(reqs[i], nreg);
    if (lvl) lvl[i] = ok ? HG_OK : HG_ERR_LEVEL;
    if (!ok && rule == WordsRule::kSkipLevelErrors) continue;
    if (!words_ok(reqs[i], nwords)) return i;
    visit(reqs[i]);
  }
  return kNoRequest;
}

}  // namespace hg
