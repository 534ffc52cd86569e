// hg_merge.hip — the rest of Handel's replace store on the device: store.go:82-99
// Store (unsafeCheckMerge :188-229 + store :264-269) for the verified picks of
// an intake step, and store.go:238-262 FullSignature / Combined
// (partitioner.go:224-296 Combine / CombineFull) for the multisignatures Handel
// sends, over the signature tables of a merge-enabled hg_stores (hg_stores.h
// StoreMergeTab). Signatures are held as their 64-byte marshals.
//
// Merge: rows (store, level) are independent, the entries of one row are
// sequential (each changes the best the next one sees). k_merge_rows names
// every entry's row; k_merge gives every entry a wave, and the wave of a row's
// first entry applies all of the row's entries in array order, so a row has
// exactly one writer and needs no atomics. The bitset algebra is lane-parallel
// (lane j owns words j, j + 64, ...: every word has one lane that reads and
// writes it); the G1 sums use bn256_curve.h's g1_add, one thread per point:
// lane j accumulates the individual signatures at bits j of the complement's
// words in Jacobian form, lanes 0 and 1 add the entry's and the best's
// signature, an LDS tree sums the 64 partial sums, and one fp_inv gives the
// affine result that is marshalled. k_merge_compact lists the changed rows in
// the order of their first entries.
//
// Combined: one wave per query. Lane k decodes level k's best signature, the
// same LDS tree sums them; level ranges are aligned power-of-two blocks clipped
// at N, so a level's words land word-aligned in the output or inside one word.
#include "hg_stores.h"

#include "bn256_curve.h"
#include "hg_packets.h"

namespace hg {

namespace {

constexpr uint32_t kNoRow = 0xffffffffu;

__device__ inline uint64_t keep_below(uint64_t v, int w, uint32_t size) {
  const uint32_t base = (uint32_t)w * 64u;
  if (base >= size) return 0;
  const uint32_t rem = size - base;
  return rem < 64 ? v & ((1ull << rem) - 1) : v;
}

__device__ inline bool store_range(const StoreTab& t, uint32_t receiver, uint32_t level, uint32_t& lo, uint32_t& hi) {
  return receiver < t.nreg && level >= 1 && level <= (uint32_t)t.levels &&
         pkt_range_level(receiver, t.nreg, (int)level, lo, hi);
}

// binomialPartitioner.rangeLevelInverse (partitioner.go:185-211): the block of
// ids that share `id`'s bits from `level - 1` up, clipped at the registry
__device__ inline bool range_level_inverse(uint32_t id, uint32_t size, int level, uint32_t& lo, uint32_t& hi) {
  const int bitsize = pkt_log2_ceil(size);
  if (level < 0 || level > bitsize + 1) return false;
  uint64_t l = 0, h = 1ull << bitsize;
  const int max_idx = level - 1;
  for (int idx = bitsize - 1; idx >= max_idx && idx >= 0 && l < h; idx--) {
    const uint64_t middle = (h + l) / 2;
    if ((id >> idx) & 1u) l = middle;
    else h = middle;
  }
  lo = (uint32_t)l;
  hi = (uint32_t)(h < size ? h : size);
  return true;
}

__device__ inline int wave_sum(int v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// a marshalled signature (4-byte aligned) as a Jacobian point; all-zero = infinity
HG_DEV void load_sig(G1J& p, const uint8_t* m) {
  bool ge, nz = false;
  fp_from_be(p.x, m, &ge, &nz);
  fp_from_be(p.y, m + 32, &ge, &nz);
  if (nz) fp_one(p.z);
  else g1_set_inf(p);
}

// The sum of the 64 lanes' points, marshalled by lane 0 into out (k_encode_g1's
// bytes). One wave per block: the barriers are the wave's own.
HG_DEV void reduce_and_marshal(G1J& acc, G1J* red, int lane, uint8_t* out) {
  red[lane] = acc;
  __syncthreads();
  for (int m = 32; m > 0; m >>= 1) {
    if (lane < m) {
      G1J a = red[lane], b = red[lane + m];
      if (!g1_is_inf(b)) {  // most lanes hold nothing
        g1_add(a, a, b);
        red[lane] = a;
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    const G1J r = red[0];
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    if (g1_is_inf(r)) {
      for (int k = 0; k < 16; k++) o[k] = 0u;
    } else {
      Fp x, y, one;
      fp_one(one);
      if (fp_eq(r.z, one)) {  // a single term: already affine
        x = r.x;
        y = r.y;
      } else {
        g1_affine(x, y, r);
      }
      fp_to_be(out, x);
      fp_to_be(out + 32, y);
    }
  }
  __syncthreads();
}

}  // namespace

// ---------------------------------------------------------------- update_sigs
__global__ __launch_bounds__(256) void k_store_update_sigs(StoreTab t, StoreMergeTab m, const hg_store_sig* recs,
                                                           int n, const uint32_t* sigs) {
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int q = threadIdx.x & 15;
  if (i >= n) return;
  const hg_store_sig r = recs[i];
  if (r.receiver >= t.nreg) return;
  const int st = t.map[r.receiver];
  if (st < 0 || st >= t.nstores) return;
  const uint32_t* src = sigs + (size_t)r.sig_off * 16;
  uint32_t* dst = nullptr;
  if (r.level == 0) {
    dst = reinterpret_cast<uint32_t*>(m.indiv_sig) + ((size_t)st * t.nreg + r.receiver) * 16;
    if (q == 0) m.own[st] = 1u;
  } else {
    uint32_t lo = 0, hi = 0;
    if (!store_range(t, r.receiver, r.level, lo, hi)) return;
    const size_t row = (size_t)st * t.levels + (r.level - 1);
    if (r.index == HG_STORE_SIG_BEST) {
      dst = reinterpret_cast<uint32_t*>(m.best_sig) + row * 16;
      if (q == 0) atomicOr(&t.flags[row], HG_STORE_BEST_SIG);
    } else {
      if (r.index >= hi - lo) return;
      dst = reinterpret_cast<uint32_t*>(m.indiv_sig) + ((size_t)st * t.nreg + lo + r.index) * 16;
      // several records of one launch may share a word of the level's set
      if (q == 0)
        atomicOr(reinterpret_cast<unsigned long long*>(m.held + row * t.stride + (r.index >> 6)),
                 1ull << (r.index & 63));
    }
  }
  dst[q] = src[q];
}

void launch_store_update_sigs(const StoreTab& t, const StoreMergeTab& m, const hg_store_sig* recs, int n,
                              const uint8_t* sigs, hipStream_t s) {
  if (n > 0) k_store_update_sigs<<<(n + 15) / 16, 256, 0, s>>>(t, m, recs, n, (const uint32_t*)sigs);
}

// ---------------------------------------------------------------- merge
// rows[e]: the row entry e is applied to, or kNoRow with results[e] final
__global__ void k_merge_rows(StoreTab t, const hg_packet* pkts, int n, const uint32_t* sel, const uint32_t* count,
                             uint32_t capacity, const int32_t* vcodes, uint32_t* rows, uint32_t* marks,
                             int32_t* results) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= capacity) return;
  uint32_t row = kNoRow;
  int32_t res = HG_MERGE_SKIPPED;
  const uint32_t cnt = count ? *count : capacity;
  if (e < cnt && vcodes[e] == HG_OK) {
    const uint32_t slot = sel[e];
    if (slot < 2u * (uint32_t)n) {
      const hg_packet P = pkts[slot >= (uint32_t)n ? slot - n : slot];
      uint32_t lo = 0, hi = 0;
      res = HG_MERGE_ERR_ROW;
      if (store_range(t, P.receiver, P.level, lo, hi)) {
        const int st = t.map[P.receiver];
        if (st >= 0 && st < t.nstores) row = (uint32_t)st * t.levels + (P.level - 1);
      }
    }
  }
  rows[e] = row;
  marks[e] = 0u;
  results[e] = res;
}

__global__ __launch_bounds__(64) void k_merge(StoreTab t, StoreMergeTab m, const hg_packet* pkts, int n,
                                             const uint32_t* sel, uint32_t capacity, int slot_stride,
                                             const uint64_t* words, const uint8_t* sigs, const uint32_t* rows,
                                             uint32_t* marks, int32_t* results) {
  __shared__ G1J red[64];
  const uint32_t e0 = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t row = rows[e0];
  if (row == kNoRow) return;
  // the row's first entry applies the row
  for (uint32_t b = 0; b < e0; b += 64) {
    const uint32_t e = b + lane;
    if (__any(e < e0 && rows[e] == row)) return;
  }
  const int st = (int)(row / (uint32_t)t.levels);
  const uint32_t level = row % (uint32_t)t.levels + 1;
  uint64_t* bw = t.tab + 2 * (size_t)row * t.stride;
  uint64_t* iw = bw + t.stride;
  uint64_t* hw = m.held + (size_t)row * t.stride;
  uint8_t* bsig = m.best_sig + (size_t)row * 64;
  uint32_t flags = t.flags[row];
  bool changed = false;
  for (uint32_t b = e0 & ~63u; b < capacity; b += 64) {
    const uint32_t ee = b + lane;
    unsigned long long todo = __ballot(ee >= e0 && ee < capacity && rows[ee] == row);
    while (todo) {
      const uint32_t e = b + (uint32_t)__builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t slot = sel[e];
      const bool individual = slot >= (uint32_t)n;
      const hg_packet P = pkts[individual ? slot - n : slot];
      uint32_t lo = 0, hi = 0;
      (void)pkt_range_level(P.receiver, t.nreg, (int)level, lo, hi);  // k_merge_rows found the range
      const uint32_t size = hi - lo;
      const int nw = (int)((size + 63) / 64);  // <= t.stride <= slot_stride
      const uint64_t* sw = words + (size_t)slot * slot_stride;
      const uint8_t* ssig = sigs + (size_t)slot * 64;
      const uint32_t idx = (uint32_t)P.origin - lo;  // the individual's mapped index
      const bool has_best = (flags & HG_STORE_HAS_BEST) != 0;

      // store.go:87-89: an individual signature's set is its one bit
      if (individual) {
        int bad = 0;
        for (int w = lane; w < nw; w += 64) {
          const uint64_t want = idx < size && (uint32_t)w == (idx >> 6) ? 1ull << (idx & 63) : 0ull;
          bad += keep_below(sw[w], w, size) != want;
        }
        if (idx >= size) bad = 1;
        if (wave_sum(bad) != 0) {
          if (lane == 0) results[e] = HG_MERGE_ERR_INDIVIDUAL;
          continue;
        }
      }

      // unsafeCheckMerge's sets (store.go:197-211); the individual's own bit
      // lies in the candidate, so whether it is in `iv` yet does not matter
      int cB = 0, cSB = 0;
      for (int w = lane; w < nw; w += 64) {
        const uint64_t sg = keep_below(sw[w], w, size);
        const uint64_t be = has_best ? bw[w] : 0ull;
        cB += __popcll(be);
        cSB += __popcll(sg & be);
      }
      cB = wave_sum(cB);
      cSB = wave_sum(cSB);
      const bool disjoint = cSB == 0;
      int cC = 0, cI = 0, cMiss = 0;
      for (int w = lane; w < nw; w += 64) {
        const uint64_t sg = keep_below(sw[w], w, size);
        const uint64_t cand = disjoint && has_best ? sg | bw[w] : sg;
        const uint64_t is = has_best ? iw[w] & ~cand : 0ull;  // without a best nothing is complemented (:190-195)
        cC += __popcll(cand);
        cI += __popcll(is);
        cMiss += __popcll(is & ~hw[w]);
      }
      cC = wave_sum(cC);
      cI = wave_sum(cI);
      cMiss = wave_sum(cMiss);
      const bool keep = !has_best || cI + cC > cB;
      if (keep && has_best && (cMiss != 0 || (disjoint && !(flags & HG_STORE_BEST_SIG)))) {
        if (lane == 0) results[e] = HG_MERGE_ERR_MISSING;  // store.go:219
        continue;
      }

      // store.go:90-91: the individual signature is kept whatever the merge decides
      if (individual) {
        if (lane < 16)
          reinterpret_cast<uint32_t*>(m.indiv_sig)[((size_t)st * t.nreg + lo + idx) * 16 + lane] =
              reinterpret_cast<const uint32_t*>(ssig)[lane];
        if ((uint32_t)lane == ((idx >> 6) & 63u)) {  // the lane that owns the word
          iw[idx >> 6] |= 1ull << (idx & 63);
          hw[idx >> 6] |= 1ull << (idx & 63);
        }
      }
      if (!keep) {
        if (lane == 0) results[e] = HG_MERGE_DISCARDED;
        __threadfence_block();
        continue;
      }

      // the candidate's signature: the entry's, the best's when merged, and iS's
      G1J acc;
      g1_set_inf(acc);
      for (int c = 0; c <= nw; c += 64) {  // chunks of 64 words; one step past the last word for the two lone terms
        uint64_t mine = 0;
        const int w = c + lane;
        if (has_best && w < nw) {
          const uint64_t sg = keep_below(sw[w], w, size);
          const uint64_t cand = disjoint ? sg | bw[w] : sg;
          mine = iw[w] & ~cand;
          bw[w] = cand | mine;
        } else if (w < nw) {
          bw[w] = keep_below(sw[w], w, size);
        } else if (w < t.stride) {
          bw[w] = 0ull;
        }
        const int steps = nw - c < 64 ? nw - c + 1 : 64;
        for (int j = 0; j < steps; j++) {
          const uint8_t* src = nullptr;
          if (c + j < nw) {
            const uint64_t word = __shfl(mine, j, 64);
            if (word == 0) continue;  // wave-uniform
            if ((word >> lane) & 1) src = m.indiv_sig + ((size_t)st * t.nreg + lo + (uint32_t)(c + j) * 64 + lane) * 64;
          } else if (lane == 0) {
            src = ssig;
          } else if (lane == 1 && has_best && disjoint) {
            src = bsig;
          }
          if (src) {
            G1J p;
            load_sig(p, src);
            g1_add(acc, acc, p);
          }
        }
      }
      for (int w = ((nw + 64) & ~63) + lane; w < t.stride; w += 64) bw[w] = 0ull;
      reduce_and_marshal(acc, red, lane, bsig);
      flags |= HG_STORE_HAS_BEST | HG_STORE_BEST_SIG;
      changed = true;
      if (lane == 0) results[e] = HG_MERGE_STORED;
      __threadfence_block();  // the next entry's lanes read what other lanes of this wave wrote
    }
  }
  if (changed && lane == 0) {
    t.flags[row] = flags;
    marks[e0] = 1u;
  }
}

// one block: changed[2 * i] = (receiver, level) of the i-th marked entry's row
__global__ __launch_bounds__(1024) void k_merge_compact(StoreTab t, const hg_packet* pkts, int n, const uint32_t* sel,
                                                        uint32_t capacity, const uint32_t* marks, uint32_t* changed,
                                                        uint32_t* nchanged) {
  __shared__ uint32_t wave_cnt[16];
  __shared__ uint32_t base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (uint32_t b = 0; b < capacity; b += 1024) {
    const uint32_t e = b + threadIdx.x;
    const bool on = e < capacity && marks[e] != 0;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = base;
    for (int k = 0; k < wv; k++) off += wave_cnt[k];
    if (on) {
      const uint32_t slot = sel[e];
      const hg_packet P = pkts[slot >= (uint32_t)n ? slot - n : slot];
      const uint32_t o = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
      changed[2 * (size_t)o] = P.receiver;
      changed[2 * (size_t)o + 1] = P.level;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = base;
      for (int k = 0; k < 16; k++) s += wave_cnt[k];
      base = s;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *nchanged = base;
}

void launch_store_merge(const StoreTab& t, const StoreMergeTab& m, const StoreMergeWs& ws, const hg_packet* pkts, int n,
                        const uint32_t* sel, const uint32_t* count, uint32_t capacity, const int32_t* vcodes,
                        int slot_stride, const uint64_t* words, const uint8_t* sigs, int32_t* results,
                        uint32_t* changed, uint32_t* nchanged, hipStream_t s) {
  if (capacity > 0) {
    k_merge_rows<<<(capacity + 255) / 256, 256, 0, s>>>(t, pkts, n, sel, count, capacity, vcodes, ws.rows, ws.marks,
                                                       results);
    k_merge<<<capacity, 64, 0, s>>>(t, m, pkts, n, sel, capacity, slot_stride, words, sigs, ws.rows, ws.marks,
                                    results);
  }
  k_merge_compact<<<1, 1024, 0, s>>>(t, pkts, n, sel, capacity, ws.marks, changed, nchanged);
}

// ---------------------------------------------------------------- combined
__global__ __launch_bounds__(64) void k_store_combined(StoreTab t, StoreMergeTab m, const hg_store_query* queries,
                                                      int nq, int out_stride, int32_t* codes, uint32_t* bitlens,
                                                      uint64_t* words, uint8_t* sigs) {
  __shared__ G1J red[64];
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  if (q >= nq) return;
  const hg_store_query Q = queries[q];
  uint64_t* ow = words + (size_t)q * out_stride;
  uint32_t* osig = reinterpret_cast<uint32_t*>(sigs + (size_t)q * 64);
  for (int w = lane; w < out_stride; w += 64) ow[w] = 0ull;
  if (lane < 16) osig[lane] = 0u;
  const bool full = Q.level == HG_STORE_LEVEL_FULL;
  const int st = Q.receiver < t.nreg ? t.map[Q.receiver] : -1;
  uint32_t gmin = 0, gmax = t.nreg;
  int32_t code = HG_OK;
  if (st < 0 || st >= t.nstores || (!full && Q.level >= (uint32_t)t.levels)) code = HG_ERR_ARG;
  else if (!full) (void)range_level_inverse(Q.receiver, t.nreg, (int)Q.level + 1, gmin, gmax);
  const uint32_t bitlen = gmax - gmin;
  if (code == HG_OK && (bitlen + 63) / 64 > (uint32_t)out_stride) code = HG_ERR_ARG;
  if (code != HG_OK) {  // wave-uniform
    if (lane == 0) {
      codes[q] = code;
      bitlens[q] = 0u;
    }
    return;
  }
  // lane k: level k of the store (0: the own signature)
  const uint32_t top = full ? (uint32_t)t.levels : Q.level;
  uint32_t lo = 0, hi = 0, fl = 0;
  size_t row = 0;
  if (lane == 0) {
    lo = Q.receiver;
    hi = lo + 1;
    fl = m.own[st] & 1u ? HG_STORE_HAS_BEST | HG_STORE_BEST_SIG : 0u;
  } else if ((uint32_t)lane <= top && store_range(t, Q.receiver, (uint32_t)lane, lo, hi)) {
    row = (size_t)st * t.levels + (lane - 1);
    fl = t.flags[row];
  }
  const bool has = (fl & HG_STORE_HAS_BEST) != 0;
  const unsigned long long has_mask = __ballot(has);
  if (__any(has && !(fl & HG_STORE_BEST_SIG))) code = HG_COMBINED_ERR_MISSING;
  else if (has_mask == 0) code = HG_COMBINED_EMPTY;
  if (code != HG_OK) {
    if (lane == 0) {
      codes[q] = code;
      bitlens[q] = 0u;
    }
    return;
  }
  // the bitset (partitioner.go:249-258, :270-276): lane j owns output words j, j + 64, ...
  const uint32_t off = lo - gmin;
  const uint32_t nwq = (bitlen + 63) / 64;
  for (uint32_t w0 = 0; w0 < nwq; w0 += 64) {
    const uint32_t w = w0 + lane;
    uint64_t v = 0;
    for (unsigned long long rest = has_mask; rest; rest &= rest - 1) {
      const int k = __builtin_ctzll(rest);
      const uint32_t koff = __shfl(off, k, 64), ksize = __shfl(hi - lo, k, 64);
      if (w >= nwq) continue;
      if (k == 0) {
        if (w == koff >> 6) v |= 1ull << (koff & 63);
        continue;
      }
      const uint64_t* kb = t.tab + 2 * ((size_t)st * t.levels + (k - 1)) * t.stride;
      const uint32_t kw = koff >> 6;
      if (ksize >= 64 || (koff & 63) == 0) {  // word-aligned block
        if (w >= kw && w - kw < (ksize + 63) / 64) v |= kb[w - kw];
      } else if (w == kw) {  // a block below 64 ids never straddles a word
        v |= kb[0] << (koff & 63);
      }
    }
    if (w < nwq) ow[w] = v;
  }
  G1J acc;
  g1_set_inf(acc);
  if (has) load_sig(acc, lane == 0 ? m.indiv_sig + ((size_t)st * t.nreg + Q.receiver) * 64 : m.best_sig + row * 64);
  reduce_and_marshal(acc, red, lane, sigs + (size_t)q * 64);
  if (lane == 0) {
    codes[q] = HG_OK;
    bitlens[q] = bitlen;
  }
}

void launch_store_combined(const StoreTab& t, const StoreMergeTab& m, const hg_store_query* queries, int nq,
                           int out_stride, int32_t* codes, uint32_t* bitlens, uint64_t* words, uint8_t* sigs,
                           hipStream_t s) {
  if (nq > 0) k_store_combined<<<nq, 64, 0, s>>>(t, m, queries, nq, out_stride, codes, bitlens, words, sigs);
}

}  // namespace hg
