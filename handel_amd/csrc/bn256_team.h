// bn256_team.h — a 16-lane "team" (one DPP row) and its Fp12 element layout.
//
// One pairing check runs on one team. Fp12 = Fp2[w]/(w^6 - xi) is kept flat
// in the team's LDS region as 12 Fp elements: element e = 2k + c holds
// component c (0 = x, the i-coefficient; 1 = y, the real part) of the Fp2
// coefficient of w^k. Lane t < 12 of the team owns element t. Lanes 12..15
// run the same instruction stream on a clamped index and never store, so the
// wave stays convergent.
//
// This header holds the team itself, the reductions of a lazy product sum
// and the element-wise Fp12 operations (conjugate, Frobenius, copy, compare,
// the inversion of a norm). The Fp12 products and squarings are not here:
// they are the generated team programs of bn256_xtab.h, run by bn256_xprog.h.
//
// The mapping to x/crypto's tower (gfP12{x,y}, gfP6{x,y,z}) is
// c0=y.z, c1=x.z, c2=y.y, c3=x.y, c4=y.x, c5=x.x; values are identical,
// only the storage order differs.
#pragma once
#include "bn256_curve.h"

namespace hg {

static constexpr int kFp12Words = 120;  // 12 elements x 10 limbs
// Fp12 slots of a team's LDS region (tools/gen_g2_schedule.py SLOTS uses the same order)
enum { S_F = 0, S_A, S_B, S_C, S_D, S_E, S_G, S_H, S_I, S_J, S_K, S_L, kSlots };

struct Team {
  uint32_t* base;  // this team's LDS slots
  int tl;          // lane within the team, 0..15
  int e;           // owned element, min(tl, 11)
  int k;           // Fp2 coefficient index e >> 1
  int comp;        // 0 = x (imag), 1 = y (real)
  bool active;     // tl < 12
  // a team spread over the kSplitWaves waves of a workgroup
  // (make_team_split): lane tl of every wave owns element e; a round's
  // products are split between the waves (bn256_xprog.h x_job_split) and
  // team_sync is a workgroup barrier. Only units built with HG_TEAM_SPLIT
  // (below) look at these fields.
  bool split;
  int wave;         // the wave within the workgroup (split teams)
  uint32_t* xchg;   // split teams: this lane's partial-column rows (kXchgWords words per other wave)
};

HG_DEV uint32_t* slot(const Team& T, int s) { return T.base + s * kFp12Words; }

HG_DEV void ld_fp(Fp& r, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.l[i] = p[i];
}
HG_DEV void st_fp(uint32_t* p, const Fp& a) {
#pragma unroll
  for (int i = 0; i < 10; i++) p[i] = a.l[i];
}
// 8-byte-aligned element access (every element of a team region: 40-byte
// stride from an 8-aligned base): 64-bit LDS operations, so a 10-limb element
// moves in 3 instructions (2 x ds_read2_b64 + ds_read_b64) instead of 5 x
// ds_read2_b32 — at one wave per SIMD every issued instruction counts.
HG_DEV void ld_fp_a8(Fp& r, const uint32_t* p) {
  const uint64_t* q = (const uint64_t*)__builtin_assume_aligned(p, 8);
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint64_t v = q[i];
    r.l[2 * i] = (uint32_t)v;
    r.l[2 * i + 1] = (uint32_t)(v >> 32);
  }
}
HG_DEV void st_fp_a8(uint32_t* p, const uint32_t* l) {
  uint64_t* q = (uint64_t*)__builtin_assume_aligned(p, 8);
#pragma unroll
  for (int i = 0; i < 5; i++) q[i] = (uint64_t)l[2 * i] | ((uint64_t)l[2 * i + 1] << 32);
}
HG_DEV void ld_fp_g8(Fp& r, const uint32_t* p) {  // the same element in HBM, as five 8-byte words
  const uint2* src = (const uint2*)__builtin_assume_aligned(p, 8);
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint2 x = src[i];
    r.l[2 * i] = x.x;
    r.l[2 * i + 1] = x.y;
  }
}
HG_DEV void st_fp_g8(uint32_t* p, const Fp& a) {
  uint2* dst = (uint2*)__builtin_assume_aligned(p, 8);
#pragma unroll
  for (int i = 0; i < 5; i++) dst[i] = make_uint2(a.l[2 * i], a.l[2 * i + 1]);
}
HG_DEV void ld_f2(Fp2& r, const uint32_t* f12, int k) {
  ld_fp(r.x, f12 + (2 * k) * 10);
  ld_fp(r.y, f12 + (2 * k + 1) * 10);
}

// Orders a team's LDS traffic: every lane's earlier LDS writes are seen by
// every lane's later LDS reads. A team lives inside ONE wave, so a wave-level
// barrier is enough (the LDS serves one wave's requests in issue order; the
// wait and the memory clobber keep the compiler from moving LDS accesses
// across it) — and a workgroup barrier would be wrong in k_verify, whose two
// waves run different programs between their shared barriers.
//
// No s_waitcnt: the LDS executes one wave's DS instructions in issue order,
// so a read issued after a write (or a write after a read) of the same wave
// sees it in that order without draining lgkmcnt; the compiler still waits
// for each loaded register before its first use. At one wave per SIMD a
// drain is a parked wave (SQ_WAIT_ANY), never hidden by another wave.
HG_DEV void team_sync() {
#ifdef HG_TEAM_SYNC_DRAIN
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
  asm volatile("" ::: "memory");
#endif
  __builtin_amdgcn_wave_barrier();
}

// Split teams exist only in translation units that define HG_TEAM_SPLIT (the
// waves per team) before their includes (bn256_sigw2.hip): everywhere else every branch on Team::split is compiled
// out, so the one-wave kernels' code is untouched.
#ifndef HG_TEAM_SPLIT
#define HG_TEAM_SPLIT 0
#endif
static constexpr bool kTeamSplit = HG_TEAM_SPLIT > 1;
static constexpr int kSplitWaves = HG_TEAM_SPLIT > 1 ? HG_TEAM_SPLIT : 1;

// team_sync for any team: a workgroup barrier when the team spans two waves
HG_DEV void team_sync(const Team& T) {
  if (kTeamSplit && T.split) __syncthreads();
  else team_sync();
}

HG_DEV Team make_team(uint32_t* lds_base, int words_per_team) {
  Team T;
  int team = (threadIdx.x & 63) >> 4;  // teams are numbered within their wave
  T.tl = threadIdx.x & 15;
  T.base = lds_base + team * words_per_team;
  T.active = T.tl < 12;
  T.e = T.active ? T.tl : 11;
  T.k = T.e >> 1;
  T.comp = T.e & 1;
  T.split = false;
  T.wave = 0;
  T.xchg = nullptr;
  return T;
}

// Four 16-lane teams over the kSplitWaves waves of a workgroup: lane tl of
// team t is lane 16 t + tl of EVERY wave; the pairing kernel's latency forms
// (bn256_sigsplit.h). xchg_base: 4 x 16 x (kSplitWaves - 1) x kXchgWords words
// of LDS after the teams' regions (the other waves' partial column sums,
// bn256_xprog.h x_job_split).
static constexpr int kXchgWords = 44;  // 21 64-bit columns, 16-byte aligned rows
HG_DEV Team make_team_split(uint32_t* lds_base, int words_per_team, uint32_t* xchg_base) {
  Team T = make_team(lds_base, words_per_team);
  const int team = (threadIdx.x & 63) >> 4;
  T.split = true;
  T.wave = threadIdx.x >> 6;
  T.xchg = xchg_base + (team * 16 + T.tl) * (kSplitWaves - 1) * kXchgWords;
  return T;
}

// Five 12-lane teams per wave (lanes 12 t .. 12 t + 11; lanes 60..63 are
// team 4's idle lanes 12..15): for programs whose pre-pass values live on
// lanes 0..11 (the generator's PRE_LANES: MUL12F), the GT fold's chunk kernel
// then runs 5 products per wave instruction stream instead of 4.
static constexpr int kTeams12 = 5;
HG_DEV int team12_index() {
  const int l = threadIdx.x & 63;
  return l < 60 ? l / 12 : 4;
}
HG_DEV Team make_team12(uint32_t* lds_base, int words_per_team) {
  Team T;
  const int team = team12_index();
  T.tl = (threadIdx.x & 63) - 12 * team;
  T.base = lds_base + team * words_per_team;
  T.active = T.tl < 12;
  T.e = T.active ? T.tl : 11;
  T.k = T.e >> 1;
  T.comp = T.e & 1;
  T.split = false;
  T.wave = 0;
  T.xchg = nullptr;
  return T;
}

// Reduce a normalized-limb value < 31p (limb 9 holds the top bits) to [0, p):
// q = floor(top / (p9 + 1)) underestimates floor(value / p) by at most one,
// so one conditional subtraction finishes.
HG_DEV void fp_reduce8(Fp& r, const uint32_t* x) {
  constexpr uint32_t p9 = p_top_limb();
  uint32_t q = x[9] / (p9 + 1u);
  uint32_t y[10];
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    int32_t v = (int32_t)x[i] - (int32_t)(q * p_limb(i)) + c;
    y[i] = (i < 9) ? ((uint32_t)v & kMask) : (uint32_t)v;
    c = v >> 26;
  }
  fp_csub(r, y);  // (the branch-guarded form measured slower here)
}

// REDC of a lazy sum that carries R-shifted linear terms (a round's linear
// terms, bn256_xprog.h): those pass through REDC unchanged, so the result is < (products / R) +
// (linear terms) + p, below 31p (generator-checked); a quotient estimate
// (fp_reduce8) makes it canonical. Sums of products only use acc_reduce.
template <int FROM = 0>
HG_DEV void acc_reduce_wide(Fp& r, Acc& a) {
  acc_redc_digits<FROM>(a);
  uint32_t x[10];
  acc_redc_limbs(x, a);
  fp_reduce8(r, x);
}

// acc_reduce_wide without the final conditional subtraction: the quotient
// estimate leaves the result in [0, 2p) (the lazy rounds, bn256_xprog.h)
template <int FROM = 0>
HG_DEV void acc_reduce_wide_lazy(Fp& r, Acc& a) {
  acc_redc_digits<FROM>(a);
  uint32_t x[10];
  acc_redc_limbs(x, a);
  constexpr uint32_t p9 = p_top_limb();
  const uint32_t q = x[9] / (p9 + 1u);
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    int32_t v = (int32_t)x[i] - (int32_t)(q * p_limb(i)) + c;
    r.l[i] = (i < 9) ? ((uint32_t)v & kMask) : (uint32_t)v;
    c = v >> 26;
  }
}

// dst = conj_p6(a): negate odd powers of w (x/crypto gfP12.Conjugate)
HG_DEV void t12_conj(const Team& T, int dst, int sa) {
  Fp v, n;
  ld_fp(v, slot(T, sa) + T.e * 10);
  fp_neg(n, v);
  fp_sel(v, (T.k & 1) != 0, n, v);
  team_sync(T);
  if (T.active) st_fp(slot(T, dst) + T.e * 10, v);
  team_sync(T);
}

__constant__ static const Fp2 kGamma1[6] = HG_GAMMA1;
__constant__ static const Fp kGamma2[6] = HG_GAMMA2;

// dst = a^p (x/crypto gfP12.Frobenius): coefficient k -> conj(a_k) * gamma1[k]
HG_DEV void t12_frob(const Team& T, int dst, int sa) {
  Fp2 X;
  ld_f2(X, slot(T, sa), T.k);
  Fp2 g = kGamma1[T.k];
  // conj(X) = (-x, y); product component comp:
  //   x: (-x) g.y + y g.x ;  y: y g.y + x g.x
  Fp nx;
  fp_neg_loose(nx, X.x);
  Acc acc;
  acc_zero(acc);
  Fp u1, u2;
  fp_sel(u1, T.comp != 0, X.y, nx);
  fp_sel(u2, T.comp != 0, X.x, X.y);
  acc_mad(acc, u1, g.y);
  acc_mad(acc, u2, g.x);
  Fp r;
  acc_reduce(r, acc);
  team_sync(T);
  if (T.active) st_fp(slot(T, dst) + T.e * 10, r);
  team_sync(T);
}

// dst = a^(p^2) (gfP12.FrobeniusP2): coefficient k -> a_k * gamma2[k] (gamma2 in Fp)
HG_DEV void t12_frob2(const Team& T, int dst, int sa) {
  Fp v;
  ld_fp(v, slot(T, sa) + T.e * 10);
  Fp g = kGamma2[T.k];
  Fp r;
  fp_mul(r, v, g);
  team_sync(T);
  if (T.active) st_fp(slot(T, dst) + T.e * 10, r);
  team_sync(T);
}

HG_DEV void t12_set_one(const Team& T, int dst) {
  Fp v;
  fp_zero(v);
  Fp one;
  fp_one(one);
  fp_sel(v, T.e == 1, one, v);  // element 1 = c0.y
  if (T.active) st_fp(slot(T, dst) + T.e * 10, v);
  team_sync(T);
}

HG_DEV void t12_copy(const Team& T, int dst, int sa) {
  Fp v;
  ld_fp(v, slot(T, sa) + T.e * 10);
  team_sync(T);
  if (T.active) st_fp(slot(T, dst) + T.e * 10, v);
  team_sync(T);
}

// true (team-uniform) when slot s equals 1
HG_DEV bool t12_is_one(const Team& T, int s) {
  Fp v, one, z;
  ld_fp(v, slot(T, s) + T.e * 10);
  fp_one(one);
  fp_zero(z);
  Fp want;
  fp_sel(want, T.e == 1, one, z);
  bool ok = fp_eq(v, want) || !T.active;
  uint64_t bal = __ballot(ok);
  int team_shift = (threadIdx.x & 63) & ~15;
  return ((bal >> team_shift) & 0xffffull) == 0xffffull;
}

// slot s2 holds N = a conj(a) (an Fp6 element over tau = w^2: odd coefficients
// zero); replaces it by N^-1 = adj(N) / d (x/crypto gfP6.Invert:
// t0 = c0^2 - xi c1 c2, t1 = xi c2^2 - c0 c1, t2 = c1^2 - c0 c2,
// d = xi (c2 t1 + c1 t2) + c0 t0). The adjugate's three products and d's
// three terms are split over lanes 0..2 with one instruction stream (lane j
// computes term j; the odd, zero coefficients of s2 carry them between lanes),
// so a lane runs 2 + 1 Fp2 products instead of 9; the Fp2 inversion of d (one
// Bernstein-Yang Fp inversion) runs on every lane, and each lane finishes
// its own element of N^-1 with one lazy sum of two products.
HG_DEV void t12_inv_norm(const Team& T, int s2) {
  uint32_t* N = slot(T, s2);
  Fp2 c0, c1, c2;
  ld_f2(c0, N, 0);
  ld_f2(c1, N, 2);
  ld_f2(c2, N, 4);
  const int j = T.tl < 3 ? T.tl : 2;
  // t_j = alpha X^2 - beta Y Z with (X, alpha; Y, Z, beta) per j
  Fp2 X, Y, Z, u, v, t;
  f2_sel(X, j == 0, c0, j == 1 ? c2 : c1);
  f2_sel(Y, j == 0, c1, c0);
  f2_sel(Z, j == 1, c1, c2);
  f2_sqr(u, X);
  f2_mul(v, Y, Z);
  Fp2 xu, xv;
  f2_mul_xi(xu, u);
  f2_mul_xi(xv, v);
  f2_sel(u, j == 1, xu, u);
  f2_sel(v, j == 0, xv, v);
  f2_sub(t, u, v);
  team_sync(T);
  if (T.tl < 3) {  // odd coefficient 2j + 1 of s2
    st_fp(N + (4 * j + 2) * 10, t.x);
    st_fp(N + (4 * j + 3) * 10, t.y);
  }
  team_sync(T);
  Fp2 t0, t1, t2;
  ld_f2(t0, N, 1);
  ld_f2(t1, N, 3);
  ld_f2(t2, N, 5);
  // term j of d: c2 t1, c1 t2, c0 t0
  Fp2 P, Q, w;
  f2_sel(P, j == 0, c2, j == 1 ? c1 : c0);
  f2_sel(Q, j == 0, t1, j == 1 ? t2 : t0);
  f2_mul(w, P, Q);
  team_sync(T);
  if (T.tl < 3) {
    st_fp(N + (4 * j + 2) * 10, w.x);
    st_fp(N + (4 * j + 3) * 10, w.y);
  }
  team_sync(T);
  Fp2 w0, w1, w2, d;
  ld_f2(w0, N, 1);
  ld_f2(w1, N, 3);
  ld_f2(w2, N, 5);
  f2_add(d, w0, w1);
  f2_mul_xi(d, d);
  f2_add(d, d, w2);
#ifndef HG_PROBE_NOINV  // timing probe only (wrong values): the inversion's share of a pairing kernel
  f2_inv(d, d);
#endif
  // element e of N^-1: component comp of t_m d^-1 (m = k / 2), zero for odd k
  const int m = T.k >> 1;
  Fp2 tm;
  f2_sel(tm, m == 0, t0, m == 1 ? t1 : t2);
  // x (imag) = tm.x d.y + tm.y d.x; y (real) = tm.y d.y - tm.x d.x
  Fp a1, b1, ntx;
  fp_neg_loose(ntx, tm.x);
  fp_sel(a1, T.comp != 0, tm.y, tm.x);
  fp_sel(b1, T.comp != 0, ntx, tm.y);
  Acc acc;
  acc_zero(acc);
  acc_mad(acc, a1, d.y);
  acc_mad(acc, b1, d.x);
  Fp e, z;
  acc_reduce(e, acc);
  fp_zero(z);
  fp_sel(e, (T.k & 1) != 0, z, e);
  team_sync(T);
  if (T.active) st_fp(N + T.e * 10, e);
  team_sync(T);
}

// t12_inv_norm in two halves around its one Fp inversion, for kernels that
// invert the norms of a whole batch of checks at once (bn256_sig12.hip: one
// batched inversion per 256 checks instead of one Bernstein-Yang inversion
// per wave, 4.3 % of the 12-lane pairing kernel's VALU instructions,
// profiles/r06p_inv_probe.json). _terms runs t12_inv_norm up to d (the
// adjugate's terms t0, t1, t2 and d, team-uniform, every lane holds them) and
// returns n = |d|^2 as f2_inv forms it; _finish, given n^-1, writes N^-1
// into slot s2 exactly as t12_inv_norm does (the same products in the same
// order: identical canonical values).
struct NormTerms {
  Fp2 t0, t1, t2, d;
};
HG_DEV void t12_inv_norm_terms(const Team& T, int s2, NormTerms& o, Fp& nrm) {
  uint32_t* N = slot(T, s2);
  Fp2 c0, c1, c2;
  ld_f2(c0, N, 0);
  ld_f2(c1, N, 2);
  ld_f2(c2, N, 4);
  const int j = T.tl < 3 ? T.tl : 2;
  Fp2 X, Y, Z, u, v, t;
  f2_sel(X, j == 0, c0, j == 1 ? c2 : c1);
  f2_sel(Y, j == 0, c1, c0);
  f2_sel(Z, j == 1, c1, c2);
  f2_sqr(u, X);
  f2_mul(v, Y, Z);
  Fp2 xu, xv;
  f2_mul_xi(xu, u);
  f2_mul_xi(xv, v);
  f2_sel(u, j == 1, xu, u);
  f2_sel(v, j == 0, xv, v);
  f2_sub(t, u, v);
  team_sync(T);
  if (T.tl < 3) {
    st_fp(N + (4 * j + 2) * 10, t.x);
    st_fp(N + (4 * j + 3) * 10, t.y);
  }
  team_sync(T);
  ld_f2(o.t0, N, 1);
  ld_f2(o.t1, N, 3);
  ld_f2(o.t2, N, 5);
  Fp2 P, Q, w;
  f2_sel(P, j == 0, c2, j == 1 ? c1 : c0);
  f2_sel(Q, j == 0, o.t1, j == 1 ? o.t2 : o.t0);
  f2_mul(w, P, Q);
  team_sync(T);
  if (T.tl < 3) {
    st_fp(N + (4 * j + 2) * 10, w.x);
    st_fp(N + (4 * j + 3) * 10, w.y);
  }
  team_sync(T);
  Fp2 w0, w1, w2;
  ld_f2(w0, N, 1);
  ld_f2(w1, N, 3);
  ld_f2(w2, N, 5);
  f2_add(o.d, w0, w1);
  f2_mul_xi(o.d, o.d);
  f2_add(o.d, o.d, w2);
  Acc acc;  // f2_inv's norm
  acc_zero(acc);
  acc_sqr(acc, o.d.x);
  acc_sqr(acc, o.d.y);
  acc_reduce(nrm, acc);
}
HG_DEV void t12_inv_norm_finish(const Team& T, int s2, const NormTerms& o, const Fp& ninv) {
  uint32_t* N = slot(T, s2);
  Fp2 d;  // d^-1, as f2_inv
  Fp ndx;
  fp_neg(ndx, o.d.x);
  fp_mul(d.x, ndx, ninv);
  fp_mul(d.y, o.d.y, ninv);
  const int m = T.k >> 1;
  Fp2 tm;  // (selects on values: a select between member references spills to scratch)
  f2_sel(tm, m == 1, o.t1, o.t2);
  f2_sel(tm, m == 0, o.t0, tm);
  Fp a1, b1, ntx;
  fp_neg_loose(ntx, tm.x);
  fp_sel(a1, T.comp != 0, tm.y, tm.x);
  fp_sel(b1, T.comp != 0, ntx, tm.y);
  Acc acc;
  acc_zero(acc);
  acc_mad(acc, a1, d.y);
  acc_mad(acc, b1, d.x);
  Fp e, z;
  acc_reduce(e, acc);
  fp_zero(z);
  fp_sel(e, (T.k & 1) != 0, z, e);
  team_sync(T);
  if (T.active) st_fp(N + T.e * 10, e);
  team_sync(T);
}

}  // namespace hg
