// hg_store_mark.h — store.go:111-183 unsafeEvaluate's arithmetic as device
// functions, for the kernels that score a slot against a store row. A slot's
// team adds six popcounts per bitset word into two 64-bit accumulators
// (mark_accumulate), reduces them with __shfl_xor, and one lane turns the sums
// into the mark (mark_from_counts). k_pool_score (hg_pool.hip, the slots of a
// standing pool) is built from all of them; k_store_evaluate (hg_stores.hip,
// the slots of a parsed batch) takes keep_below and store_range from here and
// keeps the two arithmetic steps written out, because its machine code is held
// fixed (see the comment there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hg_packets.h"
#include "hg_stores.h"

namespace hg {

constexpr int kCntBits = 21;  // a count is at most 2^16 (kStoreMaxLevels): three per accumulator
constexpr uint64_t kCntMask = (1ull << kCntBits) - 1;

// the words of a `size`-bit set: word w keeps its bits below size
static __device__ inline uint64_t keep_below(uint64_t v, int w, uint32_t size) {
  const uint32_t base = (uint32_t)w * 64u;
  if (base >= size) return 0;
  const uint32_t rem = size - base;
  return rem < 64 ? v & ((1ull << rem) - 1) : v;
}

// (receiver, level) -> the level's range among the receiver's levels
// (Partitioner.Levels = 1..ceil(log2 N), non-empty); false: no range
static __device__ inline bool store_range(const StoreTab& t, uint32_t receiver, uint32_t level, uint32_t& lo, uint32_t& hi) {
  return receiver < t.nreg && level >= 1 && level <= (uint32_t)t.levels &&
         pkt_range_level(receiver, t.nreg, (int)level, lo, hi);
}

// one word of the slot's set, the level's best and its verified individual signatures:
// acc0 += |sig| , |best| , |sig & best|;  acc1 += |sig & ind| , |sig | ind| , |sig | ind | best|
static __device__ inline void mark_accumulate(uint64_t sg, uint64_t be, uint64_t iv, uint64_t& acc0, uint64_t& acc1) {
  acc0 += (uint64_t)__popcll(sg) | (uint64_t)__popcll(be) << kCntBits | (uint64_t)__popcll(sg & be) << (2 * kCntBits);
  acc1 += (uint64_t)__popcll(sg & iv) | (uint64_t)__popcll(sg | iv) << kCntBits |
          (uint64_t)__popcll(sg | iv | be) << (2 * kCntBits);
}

// the mark of a slot of a `size`-id level from its reduced accumulators
static __device__ inline int32_t mark_from_counts(uint64_t acc0, uint64_t acc1, uint32_t size, uint32_t level, bool has_best,
                                           bool individual) {
  const int cS = (int)(acc0 & kCntMask), cB = (int)(acc0 >> kCntBits & kCntMask),
            cSB = (int)(acc0 >> (2 * kCntBits) & kCntMask);
  const int cSI = (int)(acc1 & kCntMask), cW = (int)(acc1 >> kCntBits & kCntMask),
            cF = (int)(acc1 >> (2 * kCntBits) & kCntMask);
  const int to_receive = (int)size;
  int32_t score = 0;
  if (has_best && cB == to_receive) score = 0;          // completed level
  else if (individual && cSI > 0) score = 0;            // individual signature already verified
  else if (has_best && !individual && cSB == cS) score = 0;  // the best is a superset
  else {
    int new_total, added, combine_ct;
    if (!has_best) {
      new_total = cW;
      added = new_total;
      combine_ct = new_total - cS;
    } else if (cSB > 0) {  // overlap: replace
      new_total = cW;
      added = new_total - cB;
      combine_ct = new_total - cS;
    } else {  // disjoint: merge with the verified individual signatures
      new_total = cF;
      added = new_total - cB;
      combine_ct = cF - (cB + cS);  // |final ^ (best | sig)|, best and sig disjoint
    }
    if (added <= 0) score = individual ? 1 : 0;
    else if (new_total == to_receive) score = 1000000 - (int)level * 10 - combine_ct;
    else score = 100000 - (int)level * 100 + added * 10 - combine_ct;
  }
  return score;
}

}  // namespace hg
