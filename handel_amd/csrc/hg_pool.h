// hg_pool.h — Handel's queue of parsed signatures kept in HBM across intake
// steps (hg_pool.hip): the slots readTodos (processing.go:171-220) keeps for
// its next pass, scored, picked and re-queued where they lie.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hg_stores.h"

namespace hg {

// What the later stages read of one pooled slot, beside its bitset words and
// its 64-byte signature: 32 bytes.
struct PoolRec {
  int32_t origin;
  uint32_t receiver, level;
  uint32_t flags;  // the packet's flags
  uint32_t offset, bitlen, level_size;  // the slot's request
  uint32_t individual;  // 1: the packet's individual signature
};

// One side of the pool. A slot's place in its receiver's queue is its index:
// among the slots of one receiver a lower index is earlier in the queue.
// Appending adds behind the count; a step writes the survivors to the other
// side grouped by store, each store's in its new queue order.
struct PoolSide {
  PoolRec* recs;     // capacity
  uint64_t* words;   // capacity * stride
  uint32_t* sigs;    // capacity * 16
  int32_t* marks;    // capacity: the mark of the last step, 0 for a slot appended since
  uint32_t* count;   // 1
};

// Workspaces of one pool (device pointers), sized at creation.
struct PoolWs {
  uint32_t* flags;   // capacity + 1: admission per queue position of an append, 0 last
  uint32_t* offs;    // capacity + 1: their exclusive scan
  uint64_t* keys_a;  // capacity: store << 32 | index of every slot of mark > 0
  uint64_t* keys_b;  // capacity: sorted
  uint32_t* perm;    // capacity: per store run the picks, best first, then the rest in re-queue order
  uint32_t* starts;  // nstores + 1: start of every store's run in the sorted keys
  uint32_t* picks;   // nstores + 1: min(run length, k), 0 last
  uint32_t* base;    // nstores + 1: exclusive scan of the picks
  void* temp;
  size_t temp_bytes;
};

// bytes of PoolWs::temp the sort and the scans need for `capacity` slots
hipError_t pool_temp_bytes(size_t capacity, size_t nstores, size_t* bytes);

// hg_stores_pool_append_device: the admitted slots of a parsed batch of n
// packets behind side.count, at most up to `capacity`
hipError_t launch_pool_append(const StoreTab& t, const PoolSide& side, const PoolWs& ws, uint32_t capacity,
                              const hg_packet* pkts, int n, int slot_stride, const hg_request* reqs,
                              const uint64_t* words, const uint32_t* sigs, const int32_t* codes, const uint8_t* live,
                              hipStream_t s);

// hg_stores_pool_step_device: scores `from`, writes the picks as a parsed
// batch of out_cap packets and the survivors to `to`
hipError_t launch_pool_step(const StoreTab& t, const PoolSide& from, const PoolSide& to, const PoolWs& ws,
                            uint32_t capacity, uint32_t k, uint32_t out_cap, hg_packet* out_pkts, uint32_t* sel,
                            uint32_t* count, hg_request* out_reqs, uint64_t* out_words, uint32_t* out_sigs,
                            int32_t* out_scores, hipStream_t s);

}  // namespace hg
