// hg_stores.h — device-resident Handel stores: scoring and selection of parsed
// packet slots (hg_stores.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/handel_gpu.h"

namespace hg {

// Largest registry a store set serves: a level's bit length is 16 bits on the
// wire (crypto.go:86-110), so marks stay below 2^20 and the selection key's
// fields below hold them.
constexpr int kStoreMaxLevels = 17;

// The tables of one hg_stores. Level L (1..levels) of store s is row
// r = s * levels + (L - 1): tab[2 * r * stride ...] holds the best bitset's
// `stride` words, then the verified-individual bitset's, adjacent; flags[r]
// bit 0 = the level has a best. map[id] = store index of receiver id, or -1.
struct StoreTab {
  uint64_t* tab;
  uint32_t* flags;
  const int32_t* map;
  uint32_t nreg;
  int levels;
  int stride;
  int nstores;
};

// the selection's sort key: store | 2^21 - 1 - score | queue position
constexpr int kSelPosBits = 25, kSelScoreBits = 21;
constexpr size_t kStoreMaxPackets = (size_t)1 << (kSelPosBits - 1);

// hg_stores_update's scatter: one wave per update
void launch_store_update(const StoreTab& t, const hg_store_update* ups, int n, const uint64_t* words, hipStream_t s);
// hg_stores_evaluate*: d_scores[2n]
void launch_store_evaluate(const StoreTab& t, const hg_packet* pkts, int n, int slot_stride, const uint64_t* words,
                           const int32_t* codes, const uint8_t* live, int32_t* scores, hipStream_t s);

// Workspaces of one selection over n2 = 2n slots (device pointers).
struct StoreSelectWs {
  uint64_t* keys_a;  // n2
  uint64_t* keys_b;  // n2
  uint32_t* cnt;     // nstores + 1: start of every store's run in the sorted keys
  uint32_t* picks;   // nstores + 1: min(run length, k), 0 last
  uint32_t* base;    // nstores + 1: exclusive scan of the picks
  void* temp;
  size_t temp_bytes;
};
// bytes of StoreSelectWs::temp the sort and the scan need for n2 slots
hipError_t store_select_temp_bytes(size_t n2, size_t nstores, size_t* bytes);
hipError_t launch_store_select(const StoreTab& t, const StoreSelectWs& ws, const hg_packet* pkts, int n,
                               const int32_t* scores, uint32_t k, const hg_request* reqs, const uint8_t* sigs,
                               uint32_t* sel, uint32_t* count, hg_request* out_reqs, uint8_t* out_sigs,
                               uint32_t capacity, hipStream_t s);

// ---------------------------------------------------------------- merge (hg_merge.hip)
// The signature tables of a merge-enabled hg_stores, beside StoreTab's rows:
// best_sig[64 * r]: the 64-byte marshal of row r's best (StoreTab::flags[r]
// bit 1 = known); held[r * stride ...]: the level's individual signatures that
// are held; indiv_sig[64 * (s * nreg + id)]: the individual signature of
// registry id `id` in store s, the store's own id holding the level-0 (own)
// signature; own[s] bit 0 = held.
struct StoreMergeTab {
  uint8_t* best_sig;
  uint8_t* indiv_sig;
  uint64_t* held;
  uint32_t* own;
};

// Workspaces of one merge over `capacity` entries (device pointers).
struct StoreMergeWs {
  uint32_t* rows;   // capacity: row of every applied entry, 0xffffffff otherwise
  uint32_t* marks;  // capacity: 1 at the first entry of a row whose best changed
};

// hg_stores_update_sigs' scatter: 16 lanes per record
void launch_store_update_sigs(const StoreTab& t, const StoreMergeTab& m, const hg_store_sig* recs, int n,
                              const uint8_t* sigs, hipStream_t s);
// hg_stores_merge_device: results[capacity], changed[2 * capacity], nchanged[1]
void launch_store_merge(const StoreTab& t, const StoreMergeTab& m, const StoreMergeWs& ws, const hg_packet* pkts, int n,
                        const uint32_t* sel, const uint32_t* count, uint32_t capacity, const int32_t* vcodes,
                        int slot_stride, const uint64_t* words, const uint8_t* sigs, int32_t* results,
                        uint32_t* changed, uint32_t* nchanged, hipStream_t s);
// hg_stores_combined*: one wave per query
void launch_store_combined(const StoreTab& t, const StoreMergeTab& m, const hg_store_query* queries, int nq,
                           int out_stride, int32_t* codes, uint32_t* bitlens, uint64_t* words, uint8_t* sigs,
                           hipStream_t s);

}  // namespace hg
