// hg_pool.hip — Handel's queue of parsed signatures in HBM: the slots
// readTodos (processing.go:171-220) keeps for its next pass stay on the device
// between intake steps, are scored against the stores as they are now, and the
// k best per store leave as a parsed batch for the verifier and the merge.
//
// Layout (hg_pool.h): records, bitset words, signatures and marks in separate
// arrays, two sides. Among the slots of one receiver a lower index is earlier
// in its queue; that is all the order the pool keeps.
//
// Append: an admission flag per slot in Handel's queue order, rocPRIM's
// exclusive scan, and a copy kernel (16 lanes per slot, 8-byte words) that
// writes behind the count. Nothing is written at or above the capacity.
//
// Step: k_pool_score is k_store_evaluate's team shape over pool records
// (hg_store_mark.h holds the arithmetic of both) and writes, per slot of mark
// > 0, the key store << 32 | index. After rocPRIM's radix sort every store's
// queue is one run of the keys, in queue order. k_pool_replay gives every
// store a wave that replays readTodos over its run: lane l holds the l-th best
// candidate (k <= 64 = one wave), a new mark's place is one ballot and a
// popcount, the insertion one __shfl_up; a slot that loses on arrival or is
// pushed out goes to the store's re-queue list the moment it happens. The wave
// leaves, in the run's place, the picks best first and then the re-queued
// slots in their new order. k_pool_move (16 lanes per slot) writes the picks
// as a parsed batch and the survivors to the other side, grouped by store:
// every slot's words and signature move once, every output word has one writer.
// No LDS, no atomics.
#include "hg_pool.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hg_packets.h"
#include "hg_store_mark.h"

namespace hg {

namespace {

constexpr uint64_t kKeyNone = ~0ull;
constexpr int kKeyBits = 32 + kStoreMaxLevels;  // a store index is below 2^17
constexpr int kMoveTeam = 16;

__device__ inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

}  // namespace

// ---------------------------------------------------------------- append
// q: Handel's queue position in the batch, slot = 2n's parse slot. flags[2n] = 0.
__global__ void k_pool_admit(StoreTab t, const hg_packet* pkts, int n, const int32_t* codes, const uint8_t* live,
                             uint32_t* flags) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > 2ll * n) return;
  uint32_t f = 0;
  if (q < 2ll * n) {
    const long long pkt = q >> 1;
    const long long slot = (q & 1) ? n + pkt : pkt;
    if (codes[slot] == HG_OK && (!live || live[slot] != 0)) {
      const hg_packet P = pkts[pkt];
      uint32_t lo = 0, hi = 0;
      if (store_range(t, P.receiver, P.level, lo, hi)) {
        const int st = t.map[P.receiver];
        f = st >= 0 && st < t.nstores ? 1u : 0u;
      }
    }
  }
  flags[q] = f;
}

__global__ __launch_bounds__(256) void k_pool_copy(PoolSide side, uint32_t capacity, int stride, const hg_packet* pkts,
                                                   int n, int slot_stride, const hg_request* reqs,
                                                   const uint64_t* words, const uint32_t* sigs, const uint32_t* flags,
                                                   const uint32_t* offs) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long q = tid / kMoveTeam;
  const int lane = (int)(tid % kMoveTeam);
  if (q >= 2ll * n || flags[q] == 0) return;
  const uint32_t have = min_u32(*side.count, capacity);
  const uint32_t off = offs[q];
  if (off >= capacity - have) return;  // the device-side guard: nothing at or above the capacity
  const size_t dst = (size_t)have + off;
  const long long pkt = q >> 1;
  const bool individual = (q & 1) != 0;
  const size_t slot = (size_t)(individual ? n + pkt : pkt);
  const uint64_t* sw = words + slot * slot_stride;
  uint64_t* dw = side.words + dst * stride;
  for (int w = lane; w < stride; w += kMoveTeam) dw[w] = sw[w];  // stride <= slot_stride (checked by the caller)
  side.sigs[dst * 16 + lane] = sigs[slot * 16 + lane];
  if (lane == 0) {
    const hg_packet P = pkts[pkt];
    const hg_request R = reqs[slot];
    side.recs[dst] = PoolRec{P.origin, P.receiver, P.level, P.flags, R.offset, R.bitlen, R.level_size,
                             individual ? 1u : 0u};
    side.marks[dst] = 0;
  }
}

__global__ void k_pool_bump(uint32_t* count, const uint32_t* total, uint32_t capacity) {
  const uint32_t have = min_u32(*count, capacity);
  *count = have + min_u32(*total, capacity - have);
}

hipError_t launch_pool_append(const StoreTab& t, const PoolSide& side, const PoolWs& ws, uint32_t capacity,
                              const hg_packet* pkts, int n, int slot_stride, const hg_request* reqs,
                              const uint64_t* words, const uint32_t* sigs, const int32_t* codes, const uint8_t* live,
                              hipStream_t s) {
  const size_t n2 = 2 * (size_t)n;  // <= capacity (checked by the caller): flags and offs hold n2 + 1
  k_pool_admit<<<(unsigned)((n2 + 1 + 255) / 256), 256, 0, s>>>(t, pkts, n, codes, live, ws.flags);
  size_t tb = ws.temp_bytes;
  hipError_t e = rocprim::exclusive_scan(ws.temp, tb, ws.flags, ws.offs, 0u, n2 + 1, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return e;
  k_pool_copy<<<(unsigned)((n2 * kMoveTeam + 255) / 256), 256, 0, s>>>(side, capacity, t.stride, pkts, n, slot_stride,
                                                                      reqs, words, sigs, ws.flags, ws.offs);
  k_pool_bump<<<1, 1, 0, s>>>(side.count, ws.offs + n2, capacity);
  return hipGetLastError();
}

// ---------------------------------------------------------------- step: score
// k_store_evaluate's team shape over the pool's records: tshift = log2(team),
// every lane of a wave runs the same loop count and the same shuffles.
__global__ __launch_bounds__(256) void k_pool_score(StoreTab t, PoolSide side, uint32_t capacity, uint64_t* keys,
                                                    int tshift) {
  const int team = 1 << tshift;
  const long long slot = (long long)blockIdx.x * (256 >> tshift) + (threadIdx.x >> tshift);
  const int j = threadIdx.x & (team - 1);
  const bool in_cap = slot < (long long)capacity;
  const bool in_pool = in_cap && slot < (long long)min_u32(*side.count, capacity);
  bool rd = false, individual = false, has_best = false;
  uint32_t size = 0, level = 0;
  int st = -1;
  size_t row = 0;
  if (in_pool) {
    const PoolRec R = side.recs[slot];
    uint32_t lo = 0, hi = 0;
    if (store_range(t, R.receiver, R.level, lo, hi)) {
      st = t.map[R.receiver];
      if (st >= 0 && st < t.nstores) {
        rd = true;
        individual = R.individual != 0;
        size = hi - lo;
        level = R.level;
        row = (size_t)st * t.levels + (level - 1);
        has_best = (t.flags[row] & HG_STORE_HAS_BEST) != 0;
      }
    }
  }
  const uint64_t* sw = side.words + (size_t)(in_pool ? slot : 0) * t.stride;
  const uint64_t* bw = t.tab + 2 * row * t.stride;
  const uint64_t* iw = bw + t.stride;
  uint64_t acc0 = 0, acc1 = 0;
  for (int w0 = 0; w0 < t.stride; w0 += team) {
    const int w = w0 + j;
    uint64_t sg = 0, be = 0, iv = 0;
    if (rd && w < t.stride) {
      sg = keep_below(sw[w], w, size);
      iv = keep_below(iw[w], w, size);
      if (has_best) be = keep_below(bw[w], w, size);
    }
    mark_accumulate(sg, be, iv, acc0, acc1);
  }
  for (int m = team >> 1; m > 0; m >>= 1) {
    acc0 += __shfl_xor(acc0, m, 64);
    acc1 += __shfl_xor(acc1, m, 64);
  }
  if (j != 0 || !in_cap) return;
  uint64_t key = kKeyNone;
  if (in_pool) {
    const int32_t mark = rd ? mark_from_counts(acc0, acc1, size, level, has_best, individual) : 0;
    side.marks[slot] = mark;
    if (mark > 0) key = (uint64_t)st << 32 | (uint64_t)slot;
  }
  keys[slot] = key;
}

// ---------------------------------------------------------------- step: runs
// starts[s] = first sorted index whose key belongs to store >= s (s = 0..nstores);
// picks[s] = min(run length, k), 0 last
__global__ void k_pool_runs(const uint64_t* keys, uint32_t capacity, int nstores, uint32_t k, uint32_t* starts,
                            uint32_t* picks) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nstores) return;
  uint32_t at[2];
  for (int i = 0; i < 2; i++) {
    const uint64_t want = (uint64_t)(s + i) << 32;
    uint32_t lo = 0, hi = capacity;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    at[i] = lo;
  }
  starts[s] = at[0];
  picks[s] = s < nstores ? min_u32(at[1] - at[0], k) : 0u;
}

// ---------------------------------------------------------------- step: replay
// One wave per store: readTodos over the store's queue (its run of the sorted
// keys, marks all > 0). Lane l < held holds the l-th best candidate so far.
// perm[run]: the picks, best first, then the re-queued slots in order.
__global__ __launch_bounds__(64) void k_pool_replay(const uint64_t* keys, const int32_t* marks, const uint32_t* starts,
                                                    int nstores, uint32_t k, uint32_t capacity, uint32_t* perm) {
  const int s = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (s >= nstores) return;
  const uint32_t b = min_u32(starts[s], capacity), e = min_u32(starts[s + 1], capacity);
  if (b >= e) return;  // wave-uniform
  const uint32_t len = e - b;
  uint32_t* rest = perm + b + min_u32(len, k);
  int32_t cm = 0;   // this lane's candidate: its mark
  uint32_t ci = 0;  // and its pool index
  uint32_t held = 0, nrest = 0;
  for (uint32_t c = 0; c < len; c += 64) {
    uint32_t idx = 0;
    int32_t mk = 0;
    if (c + lane < len) {
      idx = (uint32_t)keys[b + c + lane];
      if (idx < capacity) mk = marks[idx];
      else idx = 0;
    }
    const uint32_t cnt = min_u32(64u, len - c);
    for (uint32_t j = 0; j < cnt; j++) {  // everything below is wave-uniform but the candidates
      const int32_t m = __shfl(mk, (int)j, 64);
      const uint32_t i = __shfl(idx, (int)j, 64);
      if (held == k) {
        const int32_t last_m = __shfl(cm, (int)k - 1, 64);
        const uint32_t last_i = __shfl(ci, (int)k - 1, 64);
        if (lane == 0) rest[nrest] = m <= last_m ? i : last_i;  // nrest < len - min(len, k)
        nrest++;
        if (m <= last_m) continue;
        held--;
      }
      const uint32_t pos = (uint32_t)__popcll(__ballot(lane < held && cm >= m));
      const int32_t up_m = __shfl_up(cm, 1, 64);
      const uint32_t up_i = __shfl_up(ci, 1, 64);
      if (lane > pos && lane <= held) {
        cm = up_m;
        ci = up_i;
      }
      if (lane == pos) {
        cm = m;
        ci = i;
      }
      held++;
    }
  }
  if (lane < held) perm[b + lane] = ci;  // held = min(len, k)
}

// ---------------------------------------------------------------- step: move
// 16 lanes per sorted position p. p < starts[nstores]: slot perm[p] of store
// st = key >> 32, the j-th of its run: a pick (j < picks[st]) goes to entry
// base[st] + j of the output batch, a survivor to index (starts[st] - base[st])
// + (j - picks[st]) of the other side. p in [base[nstores], out_cap): filler.
__global__ __launch_bounds__(256) void k_pool_move(PoolSide from, PoolSide to, uint32_t capacity, int stride,
                                                   const uint64_t* keys, const uint32_t* perm, const uint32_t* starts,
                                                   const uint32_t* picks, const uint32_t* base, int nstores,
                                                   uint32_t out_cap, hg_packet* out_pkts, uint32_t* sel,
                                                   uint32_t* count, hg_request* out_reqs, uint64_t* out_words,
                                                   uint32_t* out_sigs, int32_t* out_scores) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long p = tid / kMoveTeam;
  const int lane = (int)(tid % kMoveTeam);
  if (p >= (long long)capacity) return;
  const uint32_t queued = min_u32(starts[nstores], capacity);
  const uint32_t total = min_u32(base[nstores], min_u32(out_cap, queued));
  if (tid == 0) {
    *count = total;
    *to.count = queued - total;
  }
  if (p < queued) {
    const uint64_t key = keys[p];
    const uint32_t st = (uint32_t)(key >> 32);
    const uint32_t idx = perm[p];
    if (st < (uint32_t)nstores && idx < capacity && starts[st] <= p) {
      const uint32_t j = (uint32_t)p - starts[st];
      const uint32_t np = picks[st];
      const uint64_t* sw = from.words + (size_t)idx * stride;
      const uint32_t sg = from.sigs[(size_t)idx * 16 + lane];
      if (j < np) {
        const uint32_t e = base[st] + j;
        if (e < total) {
          const PoolRec R = from.recs[idx];
          const uint32_t slot = R.individual ? out_cap + e : e;
          uint64_t* dw = out_words + (size_t)slot * stride;
          for (int w = lane; w < stride; w += kMoveTeam) dw[w] = sw[w];
          out_sigs[(size_t)e * 16 + lane] = sg;
          if (R.individual) out_sigs[(size_t)slot * 16 + lane] = sg;
          if (lane == 0) {
            out_pkts[e] = hg_packet{R.origin, R.receiver, R.level, R.flags, 0u, 0u, 0u, 0u};
            sel[e] = slot;
            out_reqs[e] = hg_request{R.offset, R.bitlen, R.level_size, slot * (uint32_t)stride};
            out_scores[e] = from.marks[idx];
          }
        }
      } else {
        const uint32_t d = (starts[st] - base[st]) + (j - np);
        if (d < capacity) {
          uint64_t* dw = to.words + (size_t)d * stride;
          for (int w = lane; w < stride; w += kMoveTeam) dw[w] = sw[w];
          to.sigs[(size_t)d * 16 + lane] = sg;
          if (lane == 0) {
            to.recs[d] = from.recs[idx];
            to.marks[d] = from.marks[idx];
          }
        }
      }
    }
  }
  if (p >= total && p < out_cap) {
    out_sigs[(size_t)p * 16 + lane] = 0u;
    if (lane == 0) {
      out_pkts[p] = hg_packet{0, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      sel[p] = 0xffffffffu;
      out_reqs[p] = hg_request{0u, 0u, 1u, 0u};
      out_scores[p] = 0;
    }
  }
}

hipError_t pool_temp_bytes(size_t capacity, size_t nstores, size_t* bytes) {
  size_t a = 0, b = 0, c = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, capacity, 0, kKeyBits,
                                          nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, nstores + 1,
                              rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, capacity + 1,
                              rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  *bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return hipSuccess;
}

hipError_t launch_pool_step(const StoreTab& t, const PoolSide& from, const PoolSide& to, const PoolWs& ws,
                            uint32_t capacity, uint32_t k, uint32_t out_cap, hg_packet* out_pkts, uint32_t* sel,
                            uint32_t* count, hg_request* out_reqs, uint64_t* out_words, uint32_t* out_sigs,
                            int32_t* out_scores, hipStream_t s) {
  const int S = t.nstores;
  int tshift = 0;
  while (tshift < 6 && (1 << tshift) < t.stride) tshift++;
  const size_t per_block = 256 >> tshift;
  k_pool_score<<<(unsigned)((capacity + per_block - 1) / per_block), 256, 0, s>>>(t, from, capacity, ws.keys_a, tshift);
  size_t tb = ws.temp_bytes;
  hipError_t e = rocprim::radix_sort_keys(ws.temp, tb, ws.keys_a, ws.keys_b, (size_t)capacity, 0, kKeyBits, s);
  if (e != hipSuccess) return e;
  k_pool_runs<<<(unsigned)((S + 1 + 255) / 256), 256, 0, s>>>(ws.keys_b, capacity, S, k, ws.starts, ws.picks);
  tb = ws.temp_bytes;
  e = rocprim::exclusive_scan(ws.temp, tb, ws.picks, ws.base, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return e;
  k_pool_replay<<<(unsigned)S, 64, 0, s>>>(ws.keys_b, from.marks, ws.starts, S, k, capacity, ws.perm);
  k_pool_move<<<(unsigned)(((size_t)capacity * kMoveTeam + 255) / 256), 256, 0, s>>>(
      from, to, capacity, t.stride, ws.keys_b, ws.perm, ws.starts, ws.picks, ws.base, S, out_cap, out_pkts, sel, count,
      out_reqs, out_words, out_sigs, out_scores);
  return hipGetLastError();
}

}  // namespace hg
