// bn256_gt.hip — aggregate verification in GT (the default path of
// hg_verify_aggregate and its device / multisig variants): the per-batch fold
// and comparison (FOLD team region: bn256_gtfold.h). Its tables:
// bn256_gttab.hip; the pairing: bn256_sigpair.h.
//
// processing.go:342-368 verifies a multisignature as
//     e(H, sum of the level's set keys) == e(sig, G2Base)
// (bn256/go/bn256.go:82-94). H = hashedMessage(msg) is one point per Handel
// run and the keys come from a fixed registry, so by bilinearity
//     e(H, sum pk_i) = prod e(H, pk_i)
// and every factor can be computed ONCE per (message, registry): the engine
// keeps G_i = e(H, pk_i) and, as the G2 fold does for points, the products of
// every subset of every aligned 8-key window (256 GT values per window) and of
// every aligned power-of-two block. A request then costs
//   * a GT fold: one Fp12 product per nonzero window byte of its bitset (or
//     of the bitset's complement inside an aligned block: GT values are
//     unitary, so the complement's inverse is a conjugate — no inversion,
//     no affine conversion, nothing like k_agg_finish), and
//   * ONE Miller loop (G2Base at -sig, lines from the table) plus the final
//     exponentiation, compared with the folded value: the pk-side Miller loop
//     (G2 doubling and addition programs, the pk lines) is gone.
// The verdict is the reference's for every registry of keys in G2 (keys are
// k * G2Base; the same parity scope as k_verify).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "bn256_agg.h"
#include "bn256_gt.h"
#include "bn256_gtfold.h"

namespace hg {
// ------------------------------------------------------------------ the fold of a batch
// Term encoding: bits 0..29 index a GT table, bit 30 = conjugate on load,
// bit 31 = the block table (else the window table).
static constexpr uint32_t kTermConj = 1u << 30, kTermBlk = 1u << 31, kTermIdx = kTermConj - 1;
HG_DEV const Gt* term_ptr(uint32_t t, const Gt* win, const Gt* blk) {
  return ((t & kTermBlk) ? blk : win) + (t & kTermIdx);
}

// Plan and terms (one wave per request). The pairing check compares with
//   Y = conj(agg) = prod conj(t)                 (plain fold: conj is a ring
//                                                  automorphism, so every term
//                                                  is loaded conjugated)
//   Y = conj(block * conj(prod)) = conj(block) * prod   (complemented fold:
//                                                  conj(block) is one more term)
// so a request is ONE product of m' = m + comp terms. Ranges in the batch's
// term and chunk lists are taken with atomics (their order is irrelevant);
// then the window-table index of every nonzero byte of the folded mask in
// registry-aligned windows, and the owner of each chunk. An empty bitset is
// the reference's nil-aggregate panic (HG_ERR_EMPTY_AGG).
#ifndef HG_PLAN_WAVES  // A/B knob: 4 measured slower (profiles/r05sk_small_kernels_ab.json)
#define HG_PLAN_WAVES 16
#endif
static constexpr int kPlanWaves = HG_PLAN_WAVES;  // requests per k_gt_plan workgroup (one wave each)
template <int W>
HG_DEV uint32_t nz_units(uint64_t x) {
  return W == 8 ? nz_bytes(x) : nz_halves(x);
}
// W: registry-aligned window width of the fold's table (8: the 256-entry
// tables, 16: the 65536-entry ones)
template <int W>
__global__ __launch_bounds__(64 * kPlanWaves) void k_gt_plan(const AggRequest* reqs, int n, const uint64_t* words,
                                                             int32_t* codes, int nreg, int levels, GtBlockIndex bi,
                                                             GtReq* plan, GtHdr* hdr, uint32_t* terms,
                                                             int2* ord, int cap, int chunk, int* multi) {
  constexpr uint32_t kUnits = 64 / W, kMask = (1u << W) - 1u, kShift = W == 8 ? 3 : 4;
  __shared__ int sm[kPlanWaves], sc[kPlanWaves], sb[kPlanWaves], sd[kPlanWaves], sl[kPlanWaves], ss[kPlanWaves];
  __shared__ int base_m, base_c, base_b, base_d, base_l, base_s;
  const int wv = threadIdx.x >> 6;
  const int r = blockIdx.x * kPlanWaves + wv;
  const int lane = threadIdx.x & 63;
  GtReq g;
  g.m = g.chunks = g.comp = g.k = g.term_off = g.chunk_off = 0;
  AggRequest q;
  q.offset = q.bitlen = q.level_size = q.word_offset = 0;
  bool go = r < n && codes[r] == HG_OK;
  if (go) {
    q = reqs[r];
    uint32_t cnt = 0, nzs = 0, nzu = 0;
    for (uint32_t wi = lane; wi < (q.bitlen + 63) / 64; wi += 64) cnt += __popcll(agg_word(q, words, wi));
    for (uint32_t v = lane; v < agg_nrwords_w<W>(q); v += 64) {
      nzs += nz_units<W>(agg_rword_w<W>(q, words, (int)v, false));
      nzu += nz_units<W>(agg_rword_w<W>(q, words, (int)v, true));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      cnt += __shfl_xor(cnt, d);
      nzs += __shfl_xor(nzs, d);
      nzu += __shfl_xor(nzu, d);
    }
    const AggPlan p = agg_plan(q, cnt, nzs, nzu, nreg, levels);
    if (cnt == 0) {
      if (lane == 0) codes[r] = HG_ERR_EMPTY_AGG;
      go = false;
    } else {
      g.comp = p.comp ? 1 : 0;
      g.k = p.k;
      g.m = (int)p.m + g.comp;
      g.chunks = (g.m + chunk - 1) / chunk;
    }
  }
  // ranges in the batch's term and chunk lists, and places in k_gt_combine's
  // request lists (requests of more than 4 chunks first, so the combine's
  // longest requests start first, on SIMDs of their own): one atomic per
  // workgroup and list
  const bool big = g.chunks > 4, mid = g.chunks >= 2 && g.chunks <= 4;
  // k_gt_chunks' order: every chunk longer than half the chunk size first
  // (a request's full chunks and a long tail), the short tails last, so the
  // waves of the first resident round carry the long product chains
  const int tail = g.m % chunk;
  const int nshort = (tail > 0 && 2 * tail <= chunk) ? 1 : 0, nlong = g.chunks - nshort;
  if (lane == 0) {
    sm[wv] = g.m;
    sc[wv] = g.chunks;
    sb[wv] = big ? 1 : 0;
    sd[wv] = mid ? 1 : 0;
    sl[wv] = nlong;
    ss[wv] = nshort;
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // wave 0: lanes i < kPlanWaves scan wave i's counts side by side
    const int i = threadIdx.x;
    const bool in = i < kPlanWaves;
    int v[6] = {in ? sm[i] : 0, in ? sc[i] : 0, in ? sb[i] : 0, in ? sd[i] : 0, in ? sl[i] : 0, in ? ss[i] : 0};
    int inc[6];
#pragma unroll
    for (int j = 0; j < 6; j++) inc[j] = v[j];
#pragma unroll
    for (int d = 1; d < kPlanWaves; d <<= 1) {
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const int x = __shfl_up(inc[j], d);
        if (i >= d) inc[j] += x;
      }
    }
    int tot[6];
#pragma unroll
    for (int j = 0; j < 6; j++) tot[j] = __shfl(inc[j], kPlanWaves - 1);
    if (in) {
      sm[i] = inc[0] - v[0];
      sc[i] = inc[1] - v[1];
      sb[i] = inc[2] - v[2];
      sd[i] = inc[3] - v[3];
      sl[i] = inc[4] - v[4];
      ss[i] = inc[5] - v[5];
    }
    if (i == 0) {
      // three 64-bit atomics, issued together (no branch between them): the
      // counter pairs (terms, chunks), (big, mid), (nlong, nshort) are adjacent
      // ints (little-endian halves; no low half can carry into its high one)
      typedef unsigned long long u64;
      const u64 tc2 = atomicAdd(reinterpret_cast<u64*>(&hdr->terms), (u64)(unsigned)tot[0] | ((u64)(unsigned)tot[1] << 32));
      const u64 bd2 = atomicAdd(reinterpret_cast<u64*>(&hdr->big), (u64)(unsigned)tot[2] | ((u64)(unsigned)tot[3] << 32));
      const u64 ls2 = atomicAdd(reinterpret_cast<u64*>(&hdr->nlong), (u64)(unsigned)tot[4] | ((u64)(unsigned)tot[5] << 32));
      base_m = (int)(unsigned)tc2;
      base_c = (int)(tc2 >> 32);
      base_b = (int)(unsigned)bd2;
      base_d = (int)(bd2 >> 32);
      base_l = (int)(unsigned)ls2;
      base_s = (int)(ls2 >> 32);
    }
  }
  __syncthreads();
  g.term_off = base_m + sm[wv];
  g.chunk_off = base_c + sc[wv];
  if (r < n && lane == 0) plan[r] = g;
  if (lane == 0 && big) multi[base_b + sb[wv]] = r;
  if (lane == 0 && mid) multi[n + base_d + sd[wv]] = r;
  if (!go) return;  // no barrier below
  uint32_t at = g.term_off;
  if (g.comp) {
    if (lane == 0) {
      uint32_t t;
      if (g.k <= 3) {  // a block inside one 8-key window: that window's subset entry
        const uint32_t mask = ((1u << (1u << g.k)) - 1u) << (q.offset & (uint32_t)(W - 1));
        t = (q.offset >> kShift) * (kMask + 1u) + (mask & kMask);
      } else {
        t = kTermBlk | (uint32_t)(bi.base[g.k] + (q.offset >> g.k));
      }
      terms[at] = t | kTermConj;
    }
    at++;
  }
  const uint32_t nrw = agg_nrwords_w<W>(q);
  const uint32_t win0 = q.offset >> kShift;
  const uint32_t flag = g.comp ? 0u : kTermConj;
  for (uint32_t v0 = 0; v0 < nrw; v0 += 64) {
    const uint32_t v = v0 + lane;
    const uint64_t mb = v < nrw ? agg_rword_w<W>(q, words, (int)v, g.comp != 0) : 0;
    const uint32_t pc = nz_units<W>(mb);
    uint32_t inc = pc;  // inclusive prefix over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t x = __shfl_up(inc, d);
      if (lane >= d) inc += x;
    }
    uint32_t pos = at + inc - pc;
#pragma unroll
    for (uint32_t j = 0; j < kUnits; j++) {
      const uint32_t unit = (uint32_t)(mb >> (W * j)) & kMask;
      if (unit) terms[pos++] = ((win0 + kUnits * v + j) * (kMask + 1u) + unit) | flag;
    }
    at += __shfl(inc, 63);
  }
  const int lo = base_l + sl[wv];
  for (int c = lane; c < nlong; c += 64) ord[lo + c] = make_int2(g.chunk_off + c, r);
  if (nshort && lane == 0) ord[cap - 1 - (base_s + ss[wv])] = make_int2(g.chunk_off + g.chunks - 1, r);
}

// Chunks: each team multiplies the (at most `chunk`) terms of one chunk. A
// request of one chunk is finished here (its product is Y); the others leave
// partial products for k_gt_combine. A fixed grid walks the chunk list (the
// count is on the device); every wave runs to the same, wave-uniform bound.
// The next term is fetched from HBM into registers while the current product
// runs.
static_assert(kGtChunkTeams == kTeams12, "k_gt_chunks' teams per workgroup");
// k_gt_plan's chunk schedule, as k_gt_chunks and k_tor_chunks both walk it:
// entry k is a long chunk for k < nlong (ord from 0), a short tail after (ord
// down from cap - 1); a team without a chunk (!valid) has cnt = 0.
struct FoldChunk {
  int first, cnt;  // the chunk's terms: terms[first .. first + cnt)
  int r, c;        // its request, its place in the batch's chunk list (partial[c])
  bool single;     // the request's only chunk: the product is y[r]
};
HG_DEV FoldChunk fold_chunk(bool valid, int k, int nlong, const int2* ord, int cap, const GtReq* plan, int chunk) {
  FoldChunk ch = {0, 0, 0, 0, false};
  if (valid) {
    const int2 e = k < nlong ? ord[k] : ord[cap - 1 - (k - nlong)];
    ch.c = e.x;
    ch.r = e.y;
    const GtReq g = plan[ch.r];
    ch.first = g.term_off + (ch.c - g.chunk_off) * chunk;
    ch.cnt = min(chunk, g.term_off + g.m - ch.first);
    ch.single = g.chunks == 1;
  }
  return ch;
}
// the longest chunk of the wave's teams: every team runs that many rounds
HG_DEV int wave_max(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_xor(v, d));
  return v;
}
// The chunk's term words, read once: lane tl of the team holds term tl (terms
// past 12 are read from the list), so no table read waits on a dependent index
// load. term(i), 0 past the chunk's end: i wave-uniform, every lane shuffles.
struct TermWindow {
  const uint32_t* terms;  // the batch's term list (wave-uniform)
  int first, cnt, lane0;  // the chunk's terms in it; the team's first lane in the wave
  uint32_t mine;
  HG_DEV TermWindow(const Team& T, int team, const uint32_t* terms_, const FoldChunk& ch)
      : terms(terms_), first(ch.first), cnt(ch.cnt), lane0(12 * team),
        mine(T.tl < ch.cnt ? terms_[ch.first + T.tl] : 0u) {}
  HG_DEV uint32_t operator()(int i) const {
    const uint32_t v = (uint32_t)__shfl((int)mine, lane0 + (i < 12 ? i : 0), 64);
    return i < 12 ? v : (i < cnt ? terms[first + i] : 0u);
  }
};
// minimum waves per SIMD the compiler sizes k_gt_chunks' registers for (A/B
// builds: 3 -> 168 VGPRs with 37 spills, fold alone 0.59 -> 0.66 ms,
// profiles/r05fa_fold_occupancy_ab.json; 1 = the compiler's choice, 200 VGPRs)
#ifndef HG_CHUNK_WAVES
#define HG_CHUNK_WAVES 1
#endif
__global__ __launch_bounds__(64, HG_CHUNK_WAVES) void k_gt_chunks(const Gt* win, const Gt* blk, const uint32_t* terms,
                                                  const int2* ord, int cap, const GtReq* plan, const GtHdr* hdr,
                                                  int chunk, Gt* partial, Gt* y) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);  // five 12-lane teams per wave
  fold_regs_init(T);
  const int team = team12_index();
  const int total = hdr->chunks, nlong = hdr->nlong;
  XStream S = x_stream();
  for (int base = blockIdx.x * kTeams12; base < total; base += gridDim.x * kTeams12) {  // wave-uniform
    const int k = base + team;
    const bool valid = k < total && T.active;
    const FoldChunk ch = fold_chunk(valid, k, nlong, ord, cap, plan, chunk);
    const int cnt = ch.cnt, maxc = wave_max(cnt);
    const TermWindow term(T, team, terms, ch);
    Fp cur, n1, n2, one;
    gt_one_value(one, T);
    fp_zero(n1);
    fp_zero(n2);
    const uint32_t t0 = term(0);
    gt_read(cur, term_ptr(valid ? t0 : 0u, win, blk), T);
    fp_sel(cur, valid, cur, one);
    gt_put(T, S_A, cur, valid && (t0 & kTermConj) != 0);
    // two table values in flight across the products (a read of the 16-key
    // table is a fresh HBM page most of the time)
    uint32_t t1 = term(1), t2 = term(2);
    if (1 < cnt) gt_read(n1, term_ptr(t1, win, blk), T);
    if (2 < cnt) gt_read(n2, term_ptr(t2, win, blk), T);
#pragma unroll 1
    for (int i = 1; i < maxc; i++) {
      Fp v;
      fp_sel(v, i < cnt, n1, one);
      gt_put(T, S_B, v, i < cnt && (t1 & kTermConj) != 0);
      n1 = n2;
      t1 = t2;
      t2 = term(i + 2);
      if (i + 2 < cnt) gt_read(n2, term_ptr(t2, win, blk), T);
      fold_mul(T, S);
    }
    team_sync();
    if (valid) gt_store(T, S_A, ch.single ? y + ch.r : partial + ch.c);
    team_sync();
  }
}

// Combine (one wave per request of two or more chunks): the 4 teams multiply
// every 4th partial, a 2-level tree joins them into Y.
// Workgroup b takes the b-th request of the big list, then of the mid list
// (k_gt_plan), so the requests with the longest chains are dispatched first.
__global__ __launch_bounds__(64) void k_gt_combine(int n, const GtHdr* hdr, const int* multi, const GtReq* plan,
                                                   const Gt* partial, Gt* y) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kFoldWords];
  const int b = blockIdx.x, nbig = hdr->big;
  if (b >= nbig + hdr->mid) return;  // one request per wave: uniform
  const int r = b < nbig ? multi[b] : multi[n + b - nbig];
  const GtReq g = plan[r];
  Team T = make_team(lds, kFoldWords);
  fold_regs_init(T);
  const int team = (threadIdx.x & 63) >> 4;
  XStream S = x_stream();
  const int rounds = (g.chunks + 3) / 4;
  gt_load_or_one(T, S_A, partial + (team < g.chunks ? g.chunk_off + team : 0), team < g.chunks);
  // the team's next partial in flight across the product
  Fp one, nx;
  gt_one_value(one, T);
  nx = one;
  int c = team + 4;
  if (c < g.chunks) gt_read(nx, partial + g.chunk_off + c, T);
#pragma unroll 1
  for (int i = 1; i < rounds; i++) {
    Fp v;
    fp_sel(v, c < g.chunks, nx, one);
    gt_put(T, S_B, v, false);
    c += 4;
    if (c < g.chunks) gt_read(nx, partial + g.chunk_off + c, T);
    fold_mul(T, S);
  }
  for (int d = 1; d < (g.chunks > 2 ? 4 : 2); d <<= 1) {
    team_sync();
    lds_fp12_copy(T, slot(T, S_B), lds + (team ^ d) * kFoldWords + S_A * kFp12Words);
    fold_mul(T, S);
  }
  team_sync();
  if (team == 0) gt_store(T, S_A, y + r);
}

// fe[r] == y[r] (both canonical: word equality) for every request still HG_OK;
// one wave per request, lane l < 60 compares words 2l, 2l + 1
__global__ __launch_bounds__(64) void k_gt_compare(const Gt* fe, const Gt* y, int n, int32_t* codes) {
  const int r = blockIdx.x;
  if (r >= n) return;
  const int l = threadIdx.x;
  bool eq = true;
  if (l < 60) {
    const uint2 a = reinterpret_cast<const uint2*>(fe[r].w)[l];
    const uint2 b = reinterpret_cast<const uint2*>(y[r].w)[l];
    eq = a.x == b.x && a.y == b.y;
  }
  const bool all = __ballot(!eq) == 0;
  if (l == 0 && codes[r] == HG_OK) codes[r] = all ? HG_OK : HG_ERR_SIG_INVALID;
}

// k_gt_compare plus the verdict bitset (hg_pack_verdicts_device's layout: bit
// j of byte b = request 8b + j valid), one wave per byte: the step's pack
// launch and its dependency gap fold into the comparison
__global__ __launch_bounds__(64) void k_gt_compare_bits(const Gt* fe, const Gt* y, int n, int32_t* codes,
                                                        uint8_t* bits) {
  const int b = blockIdx.x;
  const int l = threadIdx.x;
  uint2 a[8], v[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int r = min(8 * b + j, n - 1);
    a[j] = l < 60 ? reinterpret_cast<const uint2*>(fe[r].w)[l] : make_uint2(0, 0);
    v[j] = l < 60 ? reinterpret_cast<const uint2*>(y[r].w)[l] : make_uint2(0, 0);
  }
  bool mine = false;  // lane j: request 8b + j verified
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const bool all = __ballot(a[j].x != v[j].x || a[j].y != v[j].y) == 0;
    const int r = 8 * b + j;
    if (l == j && r < n) {
      int32_t c = codes[r];
      if (c == HG_OK) c = all ? HG_OK : HG_ERR_SIG_INVALID;
      codes[r] = c;
      mine = c == HG_OK;
    }
  }
  const uint64_t m = __ballot(mine);
  if (l == 0) bits[b] = (uint8_t)(m & 0xffu);
}

// ------------------------------------------------------------------ the fold over tables in torus form (bn256_gttab.hip)
using ITorF = XInst<XP_TORMULF, S_A, S_A, S_B>;  // A = A * (alpha + w), alpha in elements 0..5 of B
HG_DEV void tor_mul(const Team& T, XStream& S) {
  team_sync();
  ITorF::run(T, S, xh<ITorF>());
}
// element e of a torus entry (e < 6)
HG_DEV void tor_read(Fp& v, const Gt* g, int e) { ld_fp_g8(v, g->w + 10 * e); }
// lanes 0..5: element tl of slot B = +-alpha
HG_DEV void tor_put(const Team& T, const Fp& v0, bool conj) {
  Fp v = v0, n;
  fp_neg(n, v);
  fp_sel(v, conj, n, v);
  if (T.tl < 6) st_fp_a8(slot(T, S_B) + T.tl * 10, v.l);
}

// k_gt_chunks on a table set in torus form: the same plan, term lists, order
// and read pipeline; a team's X starts as +-alpha + w of its first term and
// takes every further term by TORMULF. Lanes 0..5 read the 240 bytes of a
// term. A team whose chunk is shorter than the wave's longest has no "one" to
// multiply by (one has no finite alpha): in such a round each lane keeps its
// element of X in slot F, which no fold program touches, and puts it back
// after the product.
__global__ __launch_bounds__(64, HG_CHUNK_WAVES) void k_tor_chunks(const Gt* win, const Gt* blk, const uint32_t* terms,
                                                   const int2* ord, int cap, const GtReq* plan, const GtHdr* hdr,
                                                   int chunk, Gt* partial, Gt* y) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);  // five 12-lane teams per wave
  fold_regs_init(T);
  const int team = team12_index();
  const int total = hdr->chunks, nlong = hdr->nlong;
  const bool rd = T.tl < 6;
  XStream S = x_stream();
  for (int base = blockIdx.x * kTeams12; base < total; base += gridDim.x * kTeams12) {  // wave-uniform
    const int k = base + team;
    const bool valid = k < total && T.active;
    const FoldChunk ch = fold_chunk(valid, k, nlong, ord, cap, plan, chunk);
    const int cnt = ch.cnt, maxc = wave_max(cnt);
    const TermWindow term(T, team, terms, ch);
    // X = +-alpha + w: element 2k + c of an even k is alpha's element k + c,
    // element 3 (the real part of w's coefficient) is one, the rest zero
    Fp cur, n1, n2, one;
    fp_one(one);
    fp_zero(cur);
    fp_zero(n1);
    fp_zero(n2);
    const uint32_t t0 = term(0);
    const bool even = (T.k & 1) == 0;
    if (valid && even) tor_read(cur, term_ptr(t0, win, blk), T.k + T.comp);
    {
      Fp n;
      fp_neg(n, cur);
      fp_sel(cur, (t0 & kTermConj) != 0, n, cur);
      fp_sel(cur, T.e == 3, one, cur);
    }
    if (T.active) st_fp_a8(slot(T, S_A) + T.e * 10, cur.l);
    uint32_t t1 = term(1), t2 = term(2);
    if (1 < cnt && rd) tor_read(n1, term_ptr(t1, win, blk), T.tl);
    if (2 < cnt && rd) tor_read(n2, term_ptr(t2, win, blk), T.tl);
#pragma unroll 1
    for (int i = 1; i < maxc; i++) {
      const bool pad = i >= cnt;
      tor_put(T, n1, (t1 & kTermConj) != 0);
      n1 = n2;
      t1 = t2;
      t2 = term(i + 2);
      if (i + 2 < cnt && rd) tor_read(n2, term_ptr(t2, win, blk), T.tl);
      if (pad) lds_fp12_copy(T, slot(T, S_F), slot(T, S_A));
      tor_mul(T, S);
      team_sync();
      if (pad) lds_fp12_copy(T, slot(T, S_A), slot(T, S_F));
    }
    team_sync();
    if (valid) gt_store(T, S_A, ch.single ? y + ch.r : partial + ch.c);
    team_sync();
  }
}

// The comparison on a table set in torus form: x[r] is the fold's X, and
// fe[r] == X/conj(X) <=> fe[r] conj(X) == X (both sides canonical: word
// equality), one 16-lane team per request and MUL12F. Codes and (bits
// non-null) the verdict bitset as k_gt_compare_bits writes them: one
// workgroup per byte, two rounds of four requests.
__global__ __launch_bounds__(64) void k_tor_compare_bits(const Gt* fe, const Gt* x, int n, int32_t* codes,
                                                         uint8_t* bits) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kFoldWords];
  Team T = make_team(lds, kFoldWords);
  fold_regs_init(T);
  const int team = (threadIdx.x & 63) >> 4;
  const int b = blockIdx.x;
  XStream S = x_stream();
  uint32_t m = 0;
#pragma unroll 1
  for (int j = 0; j < 2; j++) {
    const int r = 8 * b + 4 * j + team;
    const int ci = min(r, n - 1);
    team_sync();
    gt_load(T, S_A, fe + ci);
    gt_load(T, S_B, x + ci, true);
    fold_mul(T, S);  // A = fe conj(X)
    team_sync();
    gt_load(T, S_B, x + ci);
    team_sync();
    const bool eq = t12_equal(T, S_A, S_B);
    bool mine = false;
    if (T.tl == 0 && r < n) {
      int32_t c = codes[r];
      if (c == HG_OK) c = eq ? HG_OK : HG_ERR_SIG_INVALID;
      codes[r] = c;
      mine = c == HG_OK;
    }
    const uint64_t bal = __ballot(mine);
#pragma unroll
    for (int q = 0; q < 4; q++) m |= (uint32_t)((bal >> (16 * q)) & 1u) << (4 * j + q);
  }
  if (bits && threadIdx.x == 0) bits[b] = (uint8_t)m;
}

// ------------------------------------------------------------------ launchers
void launch_gt_fold(const AggRequest* reqs, int n, const uint64_t* words, int32_t* codes, int nreg, int levels,
                    const Gt* win, const Gt* blk, const GtBlockIndex& bi, GtWork w, Gt* y, bool zero_hdr, hipStream_t s) {
  if (n <= 0) return;
  if (w.torus && w.win_bits != 16) abort();  // a torus set has no 8-key fold table: never a classical read of it
  if (zero_hdr) (void)hipMemsetAsync(w.hdr, 0, sizeof(GtHdr), s);
  if (w.win_bits == 16)
    k_gt_plan<16><<<nblk(n, kPlanWaves), 64 * kPlanWaves, 0, s>>>(reqs, n, words, codes, nreg, levels, bi, w.plan,
                                                                  w.hdr, w.terms, w.ord, w.cap, w.chunk, w.multi);
  else
    k_gt_plan<8><<<nblk(n, kPlanWaves), 64 * kPlanWaves, 0, s>>>(reqs, n, words, codes, nreg, levels, bi, w.plan,
                                                                 w.hdr, w.terms, w.ord, w.cap, w.chunk, w.multi);
  if (w.torus)
    k_tor_chunks<<<w.chunk_grid, 64, 0, s>>>(win, blk, w.terms, w.ord, w.cap, w.plan, w.hdr, w.chunk, w.partial, y);
  else
    k_gt_chunks<<<w.chunk_grid, 64, 0, s>>>(win, blk, w.terms, w.ord, w.cap, w.plan, w.hdr, w.chunk, w.partial, y);
  k_gt_combine<<<n, 64, 0, s>>>(n, w.hdr, w.multi, w.plan, w.partial, y);
}
void launch_tor_compare(const Gt* fe, const Gt* x, int n, int32_t* codes, uint8_t* bits, hipStream_t s) {
  if (n > 0) k_tor_compare_bits<<<(n + 7) / 8, 64, 0, s>>>(fe, x, n, codes, bits);
}
void launch_gt_compare(const Gt* fe, const Gt* y, int n, int32_t* codes, hipStream_t s) {
  if (n > 0) k_gt_compare<<<n, 64, 0, s>>>(fe, y, n, codes);
}
void launch_gt_compare_bits(const Gt* fe, const Gt* y, int n, int32_t* codes, uint8_t* bits, hipStream_t s) {
  if (n > 0) k_gt_compare_bits<<<(n + 7) / 8, 64, 0, s>>>(fe, y, n, codes, bits);
}

}  // namespace hg
