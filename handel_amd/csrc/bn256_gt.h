// bn256_gt.h — data of the GT path: tables (bn256_gttab.hip), fold and comparison (bn256_gt.hip).
#pragma once
#include "bn256_kernels.h"

namespace hg {

// An Fp12 (GT) value in HBM, in the team slot layout: element e (10 limbs of
// 26 bits, Montgomery form) at w[10 e], element order of bn256_team.h.
struct Gt {
  uint32_t w[120];
};
static constexpr int kGtChunk = 8;  // default window-table values per fold chunk (one team)
static constexpr int kGtChunkTeams = 5;  // k_gt_chunks: chunks per workgroup (five 12-lane teams)
// The fold's windows: aligned 8-key windows (256 subset products each, 61 MB
// for a 4000-key registry) or 16-key windows (65536 each, 7.9 GB, built from
// the 8-key tables): GtWork.win_bits

// per-request fold plan (k_gt_plan, k_gt_scan)
struct GtReq {
  int m;          // window-table terms of the folded mask
  int chunks;     // ceil(m / chunk)
  int comp;       // folded over the complement inside the aligned block of level k
  int k;
  int term_off;   // first term in the batch's term list
  int chunk_off;  // first chunk in the batch's chunk list
};
struct alignas(8) GtHdr {
  int terms, chunks;  // one 64-bit atomic in k_gt_plan
  int big, mid;       // requests k_gt_combine finishes: > 4 chunks / 2..4 chunks (one 64-bit atomic)
  int nlong, nshort;  // chunks of more / at most half the chunk size in k_gt_chunks' order (one 64-bit atomic)
};
// level k >= 4 block j of the registry at blk[base[k] + j] (levels <= 3 are
// entries of the window table in use)
struct GtBlockIndex {
  int base[24];
};
// device workspaces of one fold launch
struct GtWork {
  GtReq* plan;
  GtHdr* hdr;
  uint32_t* terms;
  int2* ord;       // k_gt_chunks' order: (chunk, request), long chunks from 0, short ones down from cap - 1
  int cap;         // entries of ord and partial
  Gt* partial;
  int* multi;      // 2n: the big requests from 0, the mid ones from n (k_gt_combine's order)
  int chunk_grid;  // workgroups of k_gt_chunks (one wave: kGtChunkTeams teams)
  int chunk;       // terms per chunk
  int win_bits;    // 8 or 16: which window table `win` is
  bool torus;      // `win` (16-key) and `blk` are in torus form: k_tor_chunks, y[r] = X
};

// G_i = e(H, pk_i) for the n registry keys
void launch_gt_keys(const PointG2* reg, int n, const LineCoef* tab, const PointG1* h, Gt* out, hipStream_t s);
// w8[256 w + s] = product of G_{8w + j} over the bits j of s (absent keys = 1)
void launch_gt_windows8(const Gt* key, int nreg, Gt* w8, int nwin8, hipStream_t s);
// w16[65536 w + s] = product of G_{16w + j} over the bits j of s, from w8
void launch_gt_windows16(const Gt* w8, int nwin8, Gt* w16, int nwin16, hipStream_t s);
// dst[j] = src[2j] * src[2j + 1] (entries `stride` apart; a missing odd entry = 1)
void launch_gt_blocks(const Gt* src, int stride, int nsrc, Gt* dst, int ndst, hipStream_t s);
// the fold of n requests: y[r] = conj(e(H, aggregate key of r)); codes: level
// codes in, HG_ERR_EMPTY_AGG added for empty bitsets; zero_hdr: clear the
// range counters first (false: the caller's prologue did)
void launch_gt_fold(const AggRequest* reqs, int n, const uint64_t* words, int32_t* codes, int nreg, int levels,
                    const Gt* win, const Gt* blk, const GtBlockIndex& bi, GtWork w, Gt* y, bool zero_hdr,
                    hipStream_t s);
// The torus form of the 16-key window table (nwin entries) and the block table
// (nblk): each entry g = a + b w becomes alpha = (1 + a)/b in its first six
// elements, zero in the rest (bn256_gttab.hip). launch_tor_scan: *flag = 1 when an
// entry has no alpha (b = 0), else 0; nothing is written. launch_tor_convert:
// in place, only after a clean scan. A fold over converted tables (GtWork.torus)
// leaves y[r] = X with e(H, aggregate key)'s conjugate = X/conj(X), which only
// launch_tor_compare reads: fe[r] conj(X) == X for every request still HG_OK,
// and (bits non-null) the verdict bitset as launch_gt_compare_bits writes it.
void launch_tor_scan(Gt* win, size_t nwin, Gt* blk, size_t nblk, int nreg, int* flag, hipStream_t s);
void launch_tor_convert(Gt* win, size_t nwin, Gt* blk, size_t nblk, int nreg, hipStream_t s);
void launch_tor_compare(const Gt* fe, const Gt* x, int n, int32_t* codes, uint8_t* bits, hipStream_t s);
void launch_gt_compare(const Gt* fe, const Gt* y, int n, int32_t* codes, hipStream_t s);
// the same, and the verdict bitset (ceil(n / 8) bytes, hg_pack_verdicts_device's layout)
void launch_gt_compare_bits(const Gt* fe, const Gt* y, int n, int32_t* codes, uint8_t* bits, hipStream_t s);

}  // namespace hg
