// bn256_gttab.hip — the GT path's per-(message, registry) tables, which the
// fold of bn256_gt.hip reads: G_i = e(H, pk_i), the subset products of every
// aligned 8-key and 16-key window, the aligned power-of-two block products,
// the level-2 set's torus form. Team layouts: k_gt_keys k_verify's, the rest FOLD.
#include "bn256_gt.h"
#include "bn256_gtfold.h"

namespace hg {
// G_i = e(H, pk_i): the pairing team programs of k_verify with the G2Base
// pairing switched off (unit lines), then the final exponentiation.
template <int TEAMS>
__global__ __launch_bounds__(64) void k_gt_keys(const PointG2* reg, int n, const LineCoef* tab, const PointG1* hpt,
                                                Gt* out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[TEAMS * kTeamWords];
  Team T = make_team(lds, kTeamWords);
  uint32_t* F = team_regs(T);
  const int idx = blockIdx.x * TEAMS + (threadIdx.x >> 4);
  const bool valid = idx < n;
  const PointG2& Q = reg[valid ? idx : n - 1];
  CheckCtx C;
  C.qx = Q.x;
  C.qy = Q.y;
  C.hx = hpt->x;
  C.hy = hpt->y;
  C.sx = hpt->x;
  C.sy = hpt->y;
  C.use_q = Q.inf == 0;
  C.use_s = false;
  if (!C.use_q) {  // e(H, infinity) = 1: unit lines on a well-defined doubling chain
    const Fp2 gx = HG_G2X, gy = HG_G2Y;
    C.qx = gx;
    C.qy = gy;
  }
  XStream S = x_stream();
  team_miller_check(T, F, C, tab, false, S, final_exp_hint());
  team_final_exp_fc(T, F, S);  // the GT tables: FE^m (team_final_exp_fc)
  if (valid) gt_store(T, S_F, out + idx);
}

// Window subset products, first pass: for each window w and half h (keys
// 8w + 4h .. 8w + 4h + 3) the 16 products of the half's subsets, by the
// recurrence P(s) = P(s without its lowest bit) * G(lowest bit), kept in LDS;
// entries s (h = 0) and s << 4 (h = 1) of the window's table. Absent keys
// (past the registry) are 1.
__global__ __launch_bounds__(64) void k_gt_nib(const Gt* key, int nreg, int nwin, Gt* win) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kFoldWords];
  __shared__ __attribute__((aligned(16))) uint32_t dp[4][16 * kFp12Words];
  Team T = make_team(lds, kFoldWords);
  fold_regs_init(T);
  const int team = (threadIdx.x & 63) >> 4;
  const int task = blockIdx.x * 4 + team;
  const bool valid = task < 2 * nwin;
  const int w = valid ? task >> 1 : 0, h = task & 1;
  uint32_t* D = dp[team];
  XStream S = x_stream();
  Fp one;
  gt_one_value(one, T);
  if (T.active) st_fp_a8(D + T.e * 10, one.l);  // P(empty) = 1
#pragma unroll 1
  for (int s = 1; s < 16; s++) {
    const int lo = s & -s, rest = s ^ lo;
    if (rest == 0) {
      const int j = 31 - __clz(lo);
      const int kidx = 8 * w + 4 * h + j;
      gt_load_or_one(T, S_A, key + (kidx < nreg ? kidx : 0), kidx < nreg);
    } else {
      lds_fp12_copy(T, slot(T, S_A), D + rest * kFp12Words);
      lds_fp12_copy(T, slot(T, S_B), D + lo * kFp12Words);
      fold_mul(T, S);
    }
    team_sync();
    lds_fp12_copy(T, D + s * kFp12Words, slot(T, S_A));
  }
  team_sync();
  if (!valid) return;
  Gt* tw = win + (size_t)w * 256;
#pragma unroll 1
  for (int s = (h ? 1 : 0); s < 16; s++) {
    Fp v;
    ld_fp_a8(v, D + s * kFp12Words + T.e * 10);
    if (!T.active) continue;  // (st_fp_g8 written out: the helper moves this kernel's code)
    uint2* dst = (uint2*)__builtin_assume_aligned(tw[h ? s << 4 : s].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
}

// Second pass: entry (hi << 4) | lo = entry(lo) * entry(hi << 4) for hi, lo
// != 0; one team per (window, hi), 15 products.
__global__ __launch_bounds__(64) void k_gt_cross(int nwin, Gt* win) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kFoldWords];
  Team T = make_team(lds, kFoldWords);
  fold_regs_init(T);
  const int task = blockIdx.x * 4 + ((threadIdx.x & 63) >> 4);
  const bool valid = task < 15 * nwin;
  const int w = valid ? task / 15 : 0, hi = valid ? task % 15 + 1 : 1;
  Gt* tw = win + (size_t)w * 256;
  XStream S = x_stream();
#pragma unroll 1
  for (int lo = 1; lo < 16; lo++) {
    gt_load(T, S_A, tw + lo);
    gt_load(T, S_B, tw + (hi << 4));
    fold_mul(T, S);
    team_sync();
    if (valid) gt_store(T, S_A, tw + ((hi << 4) | lo));
  }
}

// 16-key windows: entry (hi << 8) | lo = w8[2w][lo] * w8[2w + 1][hi]; one
// team per (window, hi), 256 products, the next left operand in flight.
__global__ __launch_bounds__(64) void k_gt_win16(const Gt* w8, int nwin8, int nwin16, Gt* w16) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);  // five 12-lane teams per wave
  fold_regs_init(T);
  const int task = blockIdx.x * kTeams12 + team12_index();
  const bool valid = task < 256 * nwin16;
  const int w = valid ? task >> 8 : 0, hi = task & 255;
  const Gt* lo_tab = w8 + (size_t)(2 * w) * 256;
  const bool has_hi = 2 * w + 1 < nwin8;
  Gt* dst = w16 + (size_t)w * 65536 + (size_t)hi * 256;
  XStream S = x_stream();
  Fp hv, one, nxt;
  gt_one_value(one, T);
  gt_read(hv, w8 + (size_t)(has_hi ? 2 * w + 1 : 2 * w) * 256 + hi, T);
  fp_sel(hv, has_hi, hv, one);
  gt_read(nxt, lo_tab, T);
#pragma unroll 1
  for (int lo = 0; lo < 256; lo++) {
    gt_put(T, S_A, nxt, false);
    gt_put(T, S_B, hv, false);
    if (lo + 1 < 256) gt_read(nxt, lo_tab + lo + 1, T);
    fold_mul(T, S);
    team_sync();
    if (valid) gt_store(T, S_A, dst + lo);
  }
}

// Block products, one level: dst[j] = src[2j] * src[2j + 1] (the last block of
// a level may be clipped: src[2j + 1] absent -> 1). src entries `stride` apart.
__global__ __launch_bounds__(64) void k_gt_blocks(const Gt* src, int stride, int nsrc, Gt* dst, int ndst) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kFoldWords];
  Team T = make_team(lds, kFoldWords);
  fold_regs_init(T);
  const int j = blockIdx.x * 4 + ((threadIdx.x & 63) >> 4);
  const bool valid = j < ndst;
  const int a = valid ? 2 * j : 0;
  XStream S = x_stream();
  gt_load(T, S_A, src + (size_t)a * stride);
  gt_load_or_one(T, S_B, src + (size_t)(a + 1 < nsrc ? a + 1 : a) * stride, a + 1 < nsrc);
  fold_mul(T, S);
  team_sync();
  if (valid) gt_store(T, S_A, dst + j);
}

// ------------------------------------------------------------------ torus form of the fold's tables
// A table entry is unitary: g = a + b w with a, b in Fp6 = Fp2[v]/(v^3 - xi)
// (v = w^2: a holds the even powers of w, b the odd ones) and g conj(g) = 1,
// so g = (alpha + w)/(alpha - w) with alpha = (1 + a)/b. The 16-key window
// table and the block table keep alpha in the first six elements of each
// entry (the entry stride stays sizeof(Gt); the other six are zero). A running
// product is any X in Fp12 with value X/conj(X): a term multiplies it by
// (alpha + w), two Fp6 products (TORMULF) instead of an Fp12 product; the
// conjugate of a term is -alpha; partial products combine by the plain Fp12
// product (k_gt_combine, unchanged); and the check fe == X/conj(X) is
// fe conj(X) == X (k_tor_compare_bits), so nothing is inverted per request.
// g = +-1 (b = 0) has no alpha: k_tor_scan finds such entries before anything
// is written, and a table set with one stays in Fp12 form (k_gt_chunks).
struct Fp6 {
  Fp2 c[3];  // c0 + c1 v + c2 v^2
};
HG_DEV void f6_mul(Fp6& r, const Fp6& a, const Fp6& b) {
  Fp2 t0, t1, t2, s, u, w;
  Fp6 o;
  f2_mul(t0, a.c[0], b.c[0]);
  f2_mul(t1, a.c[1], b.c[1]);
  f2_mul(t2, a.c[2], b.c[2]);
  f2_add(s, a.c[1], a.c[2]);
  f2_add(u, b.c[1], b.c[2]);
  f2_mul(w, s, u);
  f2_sub(w, w, t1);
  f2_sub(w, w, t2);
  f2_mul_xi(w, w);
  f2_add(o.c[0], t0, w);  // t0 + xi (a1 b2 + a2 b1)
  f2_add(s, a.c[0], a.c[1]);
  f2_add(u, b.c[0], b.c[1]);
  f2_mul(w, s, u);
  f2_sub(w, w, t0);
  f2_sub(w, w, t1);
  f2_mul_xi(s, t2);
  f2_add(o.c[1], w, s);  // a0 b1 + a1 b0 + xi t2
  f2_add(s, a.c[0], a.c[2]);
  f2_add(u, b.c[0], b.c[2]);
  f2_mul(w, s, u);
  f2_sub(w, w, t0);
  f2_sub(w, w, t2);
  f2_add(o.c[2], w, t1);  // a0 b2 + a2 b0 + t1
  r = o;
}
// The inverse of a != 0 as adj / n: adj = a^(p^2) a^(p^4) in Fp6 and the norm
// n = a adj in Fp2, n != 0.
HG_DEV void f6_adj_norm(Fp6& adj, Fp2& n, const Fp6& a) {
  Fp2 A, B, C, t;
  f2_sqr(A, a.c[0]);
  f2_mul(t, a.c[1], a.c[2]);
  f2_mul_xi(t, t);
  f2_sub(A, A, t);  // a0^2 - xi a1 a2
  f2_sqr(B, a.c[2]);
  f2_mul_xi(B, B);
  f2_mul(t, a.c[0], a.c[1]);
  f2_sub(B, B, t);  // xi a2^2 - a0 a1
  f2_sqr(C, a.c[1]);
  f2_mul(t, a.c[0], a.c[2]);
  f2_sub(C, C, t);  // a1^2 - a0 a2
  f2_mul(n, a.c[2], B);
  f2_mul(t, a.c[1], C);
  f2_add(n, n, t);
  f2_mul_xi(n, n);
  f2_mul(t, a.c[0], A);
  f2_add(n, n, t);  // a0 A + xi (a2 B + a1 C)
  adj.c[0] = A;
  adj.c[1] = B;
  adj.c[2] = C;
}
// the Fp6 halves of an entry: odd = 0 the even powers of w (a), 1 the odd ones (b)
HG_DEV void tor_load_half(Fp6& r, const Gt* g, int odd) {
#pragma unroll
  for (int m = 0; m < 3; m++) {
    ld_fp_g8(r.c[m].x, g->w + 20 * (2 * m + odd));
    ld_fp_g8(r.c[m].y, g->w + 20 * (2 * m + odd) + 10);
  }
}
// The entries the conversion walks: the 16-key window table, then the block
// table. A window entry whose subset holds none of the registry's keys (the
// empty subset; in a ragged last window also its copies) is 1 and no request
// names it: it is skipped and keeps its bytes.
struct TorTables {
  Gt* win;
  Gt* blk;
  size_t nwin, nblk;  // entries
  int nreg;
};
HG_DEV Gt* tor_entry(const TorTables& t, size_t idx) {
  if (idx < t.nwin) {
    const int w = (int)(idx >> 16), have = min(16, t.nreg - 16 * w);
    return ((uint32_t)idx & ((1u << have) - 1u) & 0xffffu) ? t.win + idx : nullptr;
  }
  return idx < t.nwin + t.nblk ? t.blk + (idx - t.nwin) : nullptr;
}
// flag |= 1 when an entry has b = 0 (nothing is written)
__global__ __launch_bounds__(256) void k_tor_scan(TorTables t, int* flag) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const Gt* g = tor_entry(t, idx);
  if (!g) return;
  uint32_t any = 0;
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const uint4* p = reinterpret_cast<const uint4*>(g->w + 20 * (2 * m + 1));  // 80-byte offsets of a 16-aligned entry
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const uint4 v = p[i];
      any |= v.x | v.y | v.z | v.w;
    }
  }
  if (any == 0) atomicOr(flag, 1);
}
// In place, one thread per run of kTorRun consecutive entries. With
// b^-1 = adj(b) / n(b), n in Fp2, alpha = (1 + a) adj(b) / n(b): the forward
// pass leaves M = (1 + a) adj(b) in elements 0..5 of the entry, n in elements
// 6, 7 and the product of the run's earlier norms in elements 8, 9; one Fp2
// inversion per run (Montgomery's trick over the norms); the backward pass
// writes alpha = M / n to elements 0..5 and zero to the rest.
static constexpr int kTorRun = 16;
__global__ __launch_bounds__(64) void k_tor_convert(TorTables t) {
  const size_t first = ((size_t)blockIdx.x * 64 + threadIdx.x) * kTorRun;
  Fp2 acc;
  f2_one(acc);
#pragma unroll 1
  for (int i = 0; i < kTorRun; i++) {
    Gt* g = tor_entry(t, first + i);
    if (!g) continue;
    Fp6 a, b, adj;
    Fp2 n;
    tor_load_half(b, g, 1);
    f6_adj_norm(adj, n, b);
    tor_load_half(a, g, 0);
    Fp one;
    fp_one(one);
    fp_add(a.c[0].y, a.c[0].y, one);
    f6_mul(a, a, adj);
#pragma unroll
    for (int m = 0; m < 3; m++) {
      st_fp_g8(g->w + 20 * m, a.c[m].x);
      st_fp_g8(g->w + 20 * m + 10, a.c[m].y);
    }
    st_fp_g8(g->w + 60, n.x);
    st_fp_g8(g->w + 70, n.y);
    st_fp_g8(g->w + 80, acc.x);
    st_fp_g8(g->w + 90, acc.y);
    f2_mul(acc, acc, n);
  }
  Fp2 inv;
  f2_inv(inv, acc);
  Fp zero;
  fp_zero(zero);
#pragma unroll 1
  for (int i = kTorRun - 1; i >= 0; i--) {
    Gt* g = tor_entry(t, first + i);
    if (!g) continue;
    Fp2 n, pre, ni;
    ld_fp_g8(n.x, g->w + 60);
    ld_fp_g8(n.y, g->w + 70);
    ld_fp_g8(pre.x, g->w + 80);
    ld_fp_g8(pre.y, g->w + 90);
    f2_mul(ni, inv, pre);  // 1 / n_i
    f2_mul(inv, inv, n);   // the inverse of the product before i
#pragma unroll
    for (int m = 0; m < 3; m++) {
      Fp2 c;
      ld_fp_g8(c.x, g->w + 20 * m);
      ld_fp_g8(c.y, g->w + 20 * m + 10);
      f2_mul(c, c, ni);
      st_fp_g8(g->w + 20 * m, c.x);
      st_fp_g8(g->w + 20 * m + 10, c.y);
    }
#pragma unroll
    for (int e = 6; e < 12; e++) st_fp_g8(g->w + 10 * e, zero);
  }
}

// ------------------------------------------------------------------ launchers
void launch_gt_keys(const PointG2* reg, int n, const LineCoef* tab, const PointG1* h, Gt* out, hipStream_t s) {
  if (n > 0) k_gt_keys<4><<<nblk(n, 4), 64, 0, s>>>(reg, n, tab, h, out);
}
void launch_gt_windows8(const Gt* key, int nreg, Gt* w8, int nwin8, hipStream_t s) {
  if (nwin8 <= 0) return;
  k_gt_nib<<<nblk(2 * nwin8, 4), 64, 0, s>>>(key, nreg, nwin8, w8);
  k_gt_cross<<<nblk(15 * nwin8, 4), 64, 0, s>>>(nwin8, w8);
}
void launch_gt_windows16(const Gt* w8, int nwin8, Gt* w16, int nwin16, hipStream_t s) {
  if (nwin16 <= 0) return;
  k_gt_win16<<<nblk(256 * nwin16, kTeams12), 64, 0, s>>>(w8, nwin8, nwin16, w16);
}
void launch_gt_blocks(const Gt* src, int stride, int nsrc, Gt* dst, int ndst, hipStream_t s) {
  if (ndst > 0) k_gt_blocks<<<nblk(ndst, 4), 64, 0, s>>>(src, stride, nsrc, dst, ndst);
}
void launch_tor_scan(Gt* win, size_t nwin, Gt* blk, size_t nblk_, int nreg, int* flag, hipStream_t s) {
  const size_t total = nwin + nblk_;
  (void)hipMemsetAsync(flag, 0, sizeof(int), s);
  if (total) k_tor_scan<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(TorTables{win, blk, nwin, nblk_, nreg}, flag);
}
void launch_tor_convert(Gt* win, size_t nwin, Gt* blk, size_t nblk_, int nreg, hipStream_t s) {
  const size_t total = nwin + nblk_, per = 64 * kTorRun;
  if (total) k_tor_convert<<<(unsigned)((total + per - 1) / per), 64, 0, s>>>(TorTables{win, blk, nwin, nblk_, nreg});
}
}  // namespace hg
