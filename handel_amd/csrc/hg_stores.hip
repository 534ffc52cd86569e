// hg_stores.hip — Handel's scoring step on the device: store.go:111-183
// unsafeEvaluate for every parsed packet slot against device-resident stores,
// and readTodos' pick (processing.go:171-220) of the k best slots per store,
// compacted into the arrays hg_verify_aggregate_device takes.
//
// Scoring is a few popcounts per bitset word and a handful of reductions: per
// live slot it reads 3 x stride x 8 bytes (the slot's bitset, the level's best,
// the level's verified individual signatures; the latter two adjacent in one
// table row) and writes 4. HBM/L2 bound. A slot gets a team of
// min(64, next_pow2(stride)) lanes, 64 / team slots share a wave, every lane
// loads one 8-byte word per bitset per pass, and the six counts travel in two
// 64-bit accumulators through __shfl_xor inside the team. No LDS, no atomics.
//
// Selection sorts the unique keys (store, 2^21 - 1 - score, queue position) of
// the 2n slots with rocPRIM's device radix sort; the start of every store's run
// is a binary search, the output bases an exclusive scan, and one gather
// kernel writes the picks and the filler.
#include "hg_stores.h"

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hg_packets.h"
#include "hg_store_mark.h"

namespace hg {

namespace {

constexpr uint64_t kKeyNone = ~0ull;

}  // namespace

// ---------------------------------------------------------------- update
__global__ __launch_bounds__(256) void k_store_update(StoreTab t, const hg_store_update* ups, int n,
                                                      const uint64_t* words) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;  // wave-uniform
  const hg_store_update u = ups[i];
  uint32_t lo = 0, hi = 0;
  if (!store_range(t, u.receiver, u.level, lo, hi)) return;
  const int st = t.map[u.receiver];
  if (st < 0 || st >= t.nstores) return;
  const uint32_t size = hi - lo;
  const int nw = (int)((size + 63) / 64);  // <= t.stride
  const bool has = (u.flags & HG_STORE_HAS_BEST) != 0;
  const size_t row = (size_t)st * t.levels + (u.level - 1);
  uint64_t* best = t.tab + 2 * row * t.stride;
  uint64_t* indiv = best + t.stride;
  for (int w = lane; w < t.stride; w += 64) {
    const bool in = w < nw;
    best[w] = in && has ? keep_below(words[(size_t)u.best_off + w], w, size) : 0ull;
    indiv[w] = in ? keep_below(words[(size_t)u.indiv_off + w], w, size) : 0ull;
  }
  if (lane == 0) t.flags[row] = has ? HG_STORE_HAS_BEST : 0u;
}

void launch_store_update(const StoreTab& t, const hg_store_update* ups, int n, const uint64_t* words, hipStream_t s) {
  if (n > 0) k_store_update<<<(n + 3) / 4, 256, 0, s>>>(t, ups, n, words);
}

// ---------------------------------------------------------------- evaluate
// tshift = log2(team). Every lane of a wave runs the same loop count and the
// same shuffles; a slot that is not scored against a store loads nothing.
// The counts and the mark below are hg_store_mark.h's mark_accumulate and
// mark_from_counts written out: calling them here gives the same instructions
// in another register allocation, and this kernel's machine code is held fixed
// (tools/kernel_sizes.py --digest-masked). tests/test_gpu_pool.py holds the
// two against each other.
__global__ __launch_bounds__(256) void k_store_evaluate(StoreTab t, const hg_packet* pkts, int n, int slot_stride,
                                                        const uint64_t* words, const int32_t* codes,
                                                        const uint8_t* live, int32_t* scores, int tshift) {
  const int team = 1 << tshift;
  const long long slot = (long long)blockIdx.x * (256 >> tshift) + (threadIdx.x >> tshift);
  const int j = threadIdx.x & (team - 1);
  const bool in_batch = slot < 2ll * n;
  const bool individual = slot >= n;
  int32_t fixed = 0;   // the score of a slot that is not scored against a store
  bool rd = false;     // scored against row `row`
  uint32_t size = 0, level = 0;
  size_t row = 0;
  bool has_best = false;
  if (in_batch && codes[slot] == HG_OK && (!live || live[slot] != 0)) {
    const hg_packet P = pkts[individual ? slot - n : slot];
    uint32_t lo = 0, hi = 0;
    if (store_range(t, P.receiver, P.level, lo, hi)) {
      const int st = t.map[P.receiver];
      if (st < 0 || st >= t.nstores) fixed = -1;
      else {
        rd = true;
        size = hi - lo;
        level = P.level;
        row = (size_t)st * t.levels + (level - 1);
        has_best = (t.flags[row] & HG_STORE_HAS_BEST) != 0;
      }
    }
  }
  const uint64_t* sw = words + (size_t)(in_batch ? slot : 0) * slot_stride;
  const uint64_t* bw = t.tab + 2 * row * t.stride;
  const uint64_t* iw = bw + t.stride;
  // acc0 = |sig| , |best| , |sig & best|;  acc1 = |sig & ind| , |sig | ind| , |sig | ind | best|
  uint64_t acc0 = 0, acc1 = 0;
  for (int w0 = 0; w0 < t.stride; w0 += team) {
    const int w = w0 + j;
    uint64_t sg = 0, be = 0, iv = 0;
    if (rd && w < t.stride) {  // t.stride <= slot_stride (checked by the caller)
      sg = keep_below(sw[w], w, size);
      iv = keep_below(iw[w], w, size);
      if (has_best) be = keep_below(bw[w], w, size);
    }
    acc0 += (uint64_t)__popcll(sg) | (uint64_t)__popcll(be) << kCntBits | (uint64_t)__popcll(sg & be) << (2 * kCntBits);
    acc1 += (uint64_t)__popcll(sg & iv) | (uint64_t)__popcll(sg | iv) << kCntBits |
            (uint64_t)__popcll(sg | iv | be) << (2 * kCntBits);
  }
  for (int m = team >> 1; m > 0; m >>= 1) {
    acc0 += __shfl_xor(acc0, m, 64);
    acc1 += __shfl_xor(acc1, m, 64);
  }
  if (j != 0 || !in_batch) return;
  int32_t score = fixed;
  if (rd) {
    const int cS = (int)(acc0 & kCntMask), cB = (int)(acc0 >> kCntBits & kCntMask),
              cSB = (int)(acc0 >> (2 * kCntBits) & kCntMask);
    const int cSI = (int)(acc1 & kCntMask), cW = (int)(acc1 >> kCntBits & kCntMask),
              cF = (int)(acc1 >> (2 * kCntBits) & kCntMask);
    const int to_receive = (int)size;
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
  }
  scores[slot] = score;
}

void launch_store_evaluate(const StoreTab& t, const hg_packet* pkts, int n, int slot_stride, const uint64_t* words,
                           const int32_t* codes, const uint8_t* live, int32_t* scores, hipStream_t s) {
  if (n <= 0) return;
  int tshift = 0;
  while (tshift < 6 && (1 << tshift) < t.stride) tshift++;
  const long long per_block = 256 >> tshift;
  const long long blocks = (2ll * n + per_block - 1) / per_block;
  k_store_evaluate<<<(unsigned)blocks, 256, 0, s>>>(t, pkts, n, slot_stride, words, codes, live, scores, tshift);
}

// ---------------------------------------------------------------- select
__global__ void k_store_keys(StoreTab t, const hg_packet* pkts, int n, const int32_t* scores, uint64_t* keys) {
  const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= 2ll * n) return;
  const bool individual = slot >= n;
  const long long pkt = individual ? slot - n : slot;
  uint64_t key = kKeyNone;
  int32_t sc = scores[slot];
  if (sc > 0) {
    const uint32_t r = pkts[pkt].receiver;
    const int st = r < t.nreg ? t.map[r] : -1;
    if (st >= 0 && st < t.nstores) {
      const int32_t top = (1 << kSelScoreBits) - 1;
      if (sc > top) sc = top;
      key = (uint64_t)st << (kSelScoreBits + kSelPosBits) | (uint64_t)(top - sc) << kSelPosBits |
            (uint64_t)(2 * pkt + (individual ? 1 : 0));
    }
  }
  keys[slot] = key;
}

// cnt[s] = first sorted index whose key belongs to store >= s (s = 0..nstores)
__global__ void k_store_starts(const uint64_t* keys, int n2, int nstores, uint32_t* cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nstores) return;
  const uint64_t want = (uint64_t)s << (kSelScoreBits + kSelPosBits);
  int lo = 0, hi = n2;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  cnt[s] = (uint32_t)lo;
}

// starts -> picks per store: min(run length, k); entry nstores is 0
__global__ void k_store_picks(const uint32_t* starts, int nstores, uint32_t k, uint32_t* picks) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nstores) return;
  uint32_t c = 0;
  if (s < nstores) {
    c = starts[s + 1] - starts[s];
    if (c > k) c = k;
  }
  picks[s] = c;
}

// 16 lanes per entry, 4 signature bytes each. Entry e < 2n: sorted key e, if
// it is among its store's first k, goes to base[store] + rank. Entry e in
// [total, capacity): the filler.
__global__ void k_store_gather(const uint64_t* keys, int n, const uint32_t* starts, const uint32_t* base, int nstores,
                               uint32_t k, const hg_request* reqs, const uint32_t* sigs, uint32_t* sel,
                               uint32_t* count, hg_request* out_reqs, uint32_t* out_sigs, uint32_t capacity) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long e = tid >> 4;
  const int q = (int)(tid & 15);
  const long long n2 = 2ll * n;
  if (e >= n2) return;
  const uint32_t total = base[nstores];
  if (tid == 0) *count = total;
  const uint64_t key = keys[e];
  if (key != kKeyNone) {
    const uint32_t st = (uint32_t)(key >> (kSelScoreBits + kSelPosBits));
    const uint32_t rank = st < (uint32_t)nstores ? (uint32_t)e - starts[st] : k;
    if (rank < k) {
      const uint32_t pos = (uint32_t)(key & ((1ull << kSelPosBits) - 1));
      const uint32_t slot = (pos >> 1) + ((pos & 1) ? (uint32_t)n : 0u);
      const uint32_t o = base[st] + rank;  // < total <= capacity
      if (o < capacity) {
        out_sigs[(size_t)o * 16 + q] = sigs[(size_t)slot * 16 + q];
        if (q == 0) {
          sel[o] = slot;
          out_reqs[o] = reqs[slot];
        }
      }
    }
  }
  if (e >= total && e < capacity) {
    out_sigs[(size_t)e * 16 + q] = 0u;
    if (q == 0) {
      sel[e] = 0xffffffffu;
      out_reqs[e] = hg_request{0u, 0u, 1u, 0u};
    }
  }
}

hipError_t store_select_temp_bytes(size_t n2, size_t nstores, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, n2, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, nstores + 1,
                              rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  *bytes = a > b ? a : b;
  return hipSuccess;
}

hipError_t launch_store_select(const StoreTab& t, const StoreSelectWs& ws, const hg_packet* pkts, int n,
                               const int32_t* scores, uint32_t k, const hg_request* reqs, const uint8_t* sigs,
                               uint32_t* sel, uint32_t* count, hg_request* out_reqs, uint8_t* out_sigs,
                               uint32_t capacity, hipStream_t s) {
  const size_t n2 = 2 * (size_t)n;
  const int S = t.nstores;
  k_store_keys<<<(unsigned)((n2 + 255) / 256), 256, 0, s>>>(t, pkts, n, scores, ws.keys_a);
  size_t tb = ws.temp_bytes;
  hipError_t e = rocprim::radix_sort_keys(ws.temp, tb, ws.keys_a, ws.keys_b, n2, 0, 64, s);
  if (e != hipSuccess) return e;
  const unsigned sb = (unsigned)((S + 1 + 255) / 256);
  k_store_starts<<<sb, 256, 0, s>>>(ws.keys_b, (int)n2, S, ws.cnt);
  k_store_picks<<<sb, 256, 0, s>>>(ws.cnt, S, k, ws.picks);
  tb = ws.temp_bytes;
  e = rocprim::exclusive_scan(ws.temp, tb, ws.picks, ws.base, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return e;
  k_store_gather<<<(unsigned)((n2 * 16 + 255) / 256), 256, 0, s>>>(ws.keys_b, n, ws.cnt, ws.base, S, k, reqs,
                                                                   (const uint32_t*)sigs, sel, count, out_reqs,
                                                                   (uint32_t*)out_sigs, capacity);
  return hipGetLastError();
}

}  // namespace hg
