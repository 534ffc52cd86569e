// bn256_sig12.hip — the GT path's signature-side pairing on FIVE 12-lane teams
// per wave (k_verify_sig12), with the G2Base lines evaluated ahead
// (k_sig_lines).
//
// The check (processing.go:342-368 -> bn256/go/bn256.go:82-94, GT form in
// bn256_gt.hip) needs per signature FE(Miller(G2Base at -sig)). k_verify_sig
// runs it on 16-lane teams: lanes 0..11 own the twelve Fp coefficients of f,
// lanes 12..15 evaluate the next G2Base line at -sig beside f^2 — and idle
// through the final exponentiation, which is ~60 % of the kernel. Here the
// 85 line evaluations of every signature (b' = bx * x_sig, c' = cy * -y_sig:
// four Fp products per line, bn256_sigteam.h team_miller_sig) run first, as
// their own wide kernel, into HBM; the pairing kernel then needs only lanes
// 0..11 of a team, and a wave carries five checks instead of four: 20 % fewer
// wave-instructions per batch for the same per-wave program (the team
// programs are the generator's 12-lane forms: every pre-pass value on lanes
// 0..11, tools/gen_g2_schedule.py PRE_LANES).
//
// Evaluated lines in HBM: ev[(s * n + c) * 4 + j], j = FB.x, FB.y, FC.x, FC.y
// of line s for check c (160 bytes; a wave's five teams read 800 contiguous
// bytes per line). 85 lines x 160 B = 13.6 KB per check. k_sig_scalars
// decodes each signature once, k_sig_lines runs one product per thread (n x
// 340 threads: the whole GPU, a few microseconds per batch).
//
// Two lines that follow each other with nothing between (a nonzero NAF
// digit's doubling and addition lines, 18 times, and the two Frobenius lines)
// are multiplied into f as ONE factor of five coefficients (PairCoef,
// bn256_kernels.h; the generator's LINE2_FIX_12): one round of 9 products per
// lane and no linear term where two line rounds ran 4 + 4 and a linear term,
// each with its own pre-pass, REDC and tail. Such a pair's two rows of ev
// hold L0, L1 and L2, L4 instead of the two lines, so the 13.6 KB per check
// stay.
//
// Team region (layout T, tools/gen_g2_schedule.py): five Fp12 slots and the
// register file, 92 elements (kSigTTeamElems; 94 before the shared-operand
// squaring of r06) — the final exponentiation parks two of its seven live
// values in HBM (bn256_sigfe.h team_final_exp_fc_t) — so a wave of five teams
// takes 18.4 KB of LDS and a CU holds eight pairing waves (two per SIMD: the
// unpadded kernels' 193-212 VGPRs allow it) beside a fold
// workgroup.
//
// The Miller value differs from k_verify_sig's by an Fp2 factor (the pairs'
// normalisation), which the final exponentiation removes: the FE values are
// the same field elements, canonical, so their bytes and every verdict are
// k_verify_sig's (tests/test_gpu_line_pairs.py). One exception, in a value
// nobody compares: a signature that fails to decode gets the scalars of
// infinity here (k_sig_scalars), hence FE = 1, where k_verify_sig runs on
// whatever its coordinates give; its verdict is the decode error either way.
#include <hip/hip_runtime.h>

#include "bn256_decode.h"
#include "bn256_regs.h"
#include "bn256_sigfe.h"
#include "bn256_sigpair.h"

namespace hg {

// threads per workgroup of the two small kernels ahead of the pairing (A/B
// knob: 64 measured slower, profiles/r05sk_small_kernels_ab.json)
#ifndef HG_SIG_LINE_BLOCK
#define HG_SIG_LINE_BLOCK 256
#endif
static constexpr int kLineBlock = HG_SIG_LINE_BLOCK;

// How team_miller_sig12 consumes line s of the table: alone, or as the first
// or second line of a pair (PairCoef `pair`, bn256_kernels.h). From the NAF of
// 6u + 2, like k_g2_lines' walk.
enum : uint8_t { kRowSingle = 0, kRowPairFirst = 1, kRowPairSecond = 2 };
struct SigRowMap {
  uint8_t kind[kNumLines], pair[kNumLines];
};
constexpr SigRowMap sig_row_map() {
  constexpr int8_t naf[kNafLen] = HG_NAF;
  SigRowMap m{};
  int s = 0, p = 0;
  for (int i = kNafLen - 1; i > 0; i--) {
    if (naf[i - 1] != 0) {
      m.kind[s] = kRowPairFirst;
      m.kind[s + 1] = kRowPairSecond;
      m.pair[s] = m.pair[s + 1] = (uint8_t)p++;
      s += 2;
    } else {
      m.kind[s++] = kRowSingle;
    }
  }
  m.kind[s] = kRowPairFirst;  // the two Frobenius lines
  m.kind[s + 1] = kRowPairSecond;
  m.pair[s] = m.pair[s + 1] = (uint8_t)p;
  return m;
}
static constexpr SigRowMap kSigRows = sig_row_map();
__constant__ static const SigRowMap kSigRowsDev = sig_row_map();  // k_sig_lines reads it by blockIdx.y
static_assert(kSigRows.kind[0] == kRowSingle, "team_miller_sig12 seeds f with line 0, a line of its own");
static_assert(kSigRows.pair[kNumLines - 1] == kNumPairs - 1, "kNumPairs");

// the signature's evaluation scalars: sc[5c ..] = x, y', y'^2, x y', x^2 with
// x = x_sig, y' = -y_sig. All 0 at infinity — e(inf, G2Base) = 1: every line
// then evaluates to w^3 and every pair to the Fp2 constant xi / K3, which the
// final exponentiation maps to 1 — and for a signature that fails to decode,
// whose FE value is never compared (its code is the decode error,
// k_agg_prologue).
static constexpr int kSigScalars = 5;
__global__ __launch_bounds__(kLineBlock) void k_sig_scalars(const uint8_t* sig_bytes, int flavor, int n, Fp* sc) {
  const int c = blockIdx.x * kLineBlock + threadIdx.x;
  if (c >= n) return;
  PointG1 sg;
  const int32_t code = decode_g1_one(sig_bytes + (size_t)c * 64, flavor, sg);
  Fp x, y, nsy, z;
  fp_zero(z);
  fp_neg(nsy, sg.y);
  const bool use = sg.inf == 0 && code == HG_OK;
  fp_sel(x, use, sg.x, z);
  fp_sel(y, use, nsy, z);
  Fp* o = sc + (size_t)kSigScalars * c;
  o[0] = x;
  o[1] = y;
  fp_sqr(o[2], y);
  fp_mul(o[3], x, y);
  fp_sqr(o[4], x);
}

// ev[(s * n + c) * 4 + j]: row s of check c. A line of its own: component j of
// line s at -sig_c (FB = bx x, FC = cy y'). A pair's two rows: L0, L1 then L2,
// L4 of PairCoef's L (x, y each). One Montgomery product per thread (L0 adds
// its constant); grid (4n / 256, lines), consecutive threads on consecutive
// 40-byte results
__global__ __launch_bounds__(kLineBlock) void k_sig_lines(const Fp* sc, int n, const LineCoef* tab, Fp* ev) {
  const int t = blockIdx.x * kLineBlock + threadIdx.x;  // 4 c + j
  if (t >= 4 * n) return;
  const int s = blockIdx.y;
  const int kind = kSigRowsDev.kind[s];
  const int j = t & 3;
  const int c = t >> 2;
  const Fp* v = sc + (size_t)kSigScalars * c;
  Fp o;
  if (kind == kRowSingle) {
    fp_mul(o, reinterpret_cast<const Fp*>(&tab[s])[j], v[j >> 1]);
  } else {
    const Fp* pc = reinterpret_cast<const Fp*>(&line_pairs(tab)[kSigRowsDev.pair[s]]);  // k0, xi, k1, k2, k4 (x, y each)
    if (kind == kRowPairFirst) {
      fp_mul(o, pc[j < 2 ? j : 2 + j], v[j < 2 ? 2 : 3]);  // k0 y'^2, k1 x y'
      if (j < 2) fp_add(o, o, pc[2 + j]);                  // + xi / K3
    } else {
      fp_mul(o, pc[6 + j], v[j < 2 ? 4 : 0]);  // k2 x^2, k4 x
    }
  }
  st_fp_g8(ev[(size_t)s * 4 * n + t].l, o);
}

// The evaluated rows reach the team's registers through one VGPR element per
// lane, read from HBM one publication ahead so the read's latency overlaps the
// rounds between: a line of its own (cnt = 4) from lanes 0..3 into FB, FC; a
// pair (cnt = 8: rows s, s + 1) from lanes 0..7 into FBX, FCY, FB, FC, the
// generator's LINE2_REGS (L0, L1, L2, L4).
static_assert(R_FCY_x == R_FBX_x + 2 && R_FB_x == R_FBX_x + 4 && R_FC_x == R_FBX_x + 6, "LINE2_REGS are consecutive");
struct EvPipe {
  Fp c;
};
HG_DEV void ev_fetch(const Team& T, EvPipe& P, const Fp* ev, int n, int ci, int s, int cnt) {
  if (T.tl < cnt) ld_fp_g8(P.c, ev[((size_t)(s + (T.tl >> 2)) * n + ci) * 4 + (T.tl & 3)].l);
}
// the held rows into the registers, then the cnt_next rows from `next` on into
// flight (cnt_next = 0: none left)
HG_DEV void ev_publish(const Team& T, uint32_t* F, EvPipe& P, const Fp* ev, int n, int ci, int cnt, int next,
                       int cnt_next) {
  if (T.tl < cnt) st_fp_a8(F + ((cnt == 8 ? R_FBX_x : R_FB_x) + T.tl) * 10, P.c.l);
  team_sync();
  if (cnt_next > 0) ev_fetch(T, P, ev, n, ci, next, cnt_next);
}

using ISqr12T = XInst<XP_SQR12_12_T, S_F, S_F>;
using ILineT = XInst<XP_LINE_FIX_12_T, S_F, S_F>;
using ILine2T = XInst<XP_LINE2_FIX_12_T, S_F, S_F>;

// Miller(G2Base at -sig) over the NAF of 6u + 2 (bn256_sigteam.h
// team_miller_sig's loop; the rows arrive evaluated), up to an Fp2 factor that
// the final exponentiation removes: f starts as the first line (not as 1,
// squared and multiplied by it); then per digit f^2 and f * line, on a
// nonzero digit f * (the doubling's line * the addition's) in ONE round
// (LINE2_FIX_12); then the two Frobenius lines, one round as well.
HG_DEV void team_miller_sig12(const Team& T, uint32_t* F, const Fp* ev, const Fp* sc, int n, int ci, XStream& S,
                              XHint after) {
  const int8_t naf[kNafLen] = HG_NAF;
  {
    // f = FC + FB w + w^3 of row 0: element e < 4 is the row's component e ^ 2
    Fp v, one;
    fp_zero(v);
    fp_one(one);
    if (T.tl < 4) ld_fp_g8(v, ev[(size_t)ci * 4 + (T.tl ^ 2)].l);
    fp_sel(v, T.e == 7, one, v);  // element 7 = c3.y
    if (T.active) st_fp_a8(slot(T, S_F) + T.e * 10, v.l);
  }
  if (T.tl == 0) {
    Fp zero, one;
    fp_zero(zero);
    fp_one(one);
    st_fp(F + R_ZERO * 10, zero);
    st_fp(F + R_ONE * 10, one);
  }
  if (T.tl == 1) {  // y', the pairs' w^3 coefficient
    Fp y;
    ld_fp_g8(y, sc[(size_t)kSigScalars * ci + 1].l);
    st_fp_a8(F + R_NSY * 10, y.l);
  }
  EvPipe P;
  fp_zero(P.c);
  int s = 1;
  ev_fetch(T, P, ev, n, ci, s, naf[kNafLen - 3] != 0 ? 8 : 4);
  for (int i = kNafLen - 2; i > 0; i--) {
    const int d = naf[i - 1];
    const int cnt = d != 0 ? 8 : 4;
    const int next = s + (cnt >> 2);
    // what the following digit reads; after the last one, the Frobenius pair
    const int cnt_next = i > 1 && naf[i - 2] == 0 ? 4 : 8;
    ev_publish(T, F, P, ev, n, ci, cnt, next, cnt_next);  // read by the product after f^2
    ISqr12T::run(T, S, d != 0 ? xh<ILine2T>() : xh<ILineT>());
    const XHint after_digit = i > 1 ? xh<ISqr12T>() : xh<ILine2T>();
    if (d != 0) ILine2T::run(T, S, after_digit);
    else ILineT::run(T, S, after_digit);
    s = next;
  }
  // the two Frobenius lines
  ev_publish(T, F, P, ev, n, ci, 8, kNumLines, 0);
  ILine2T::run(T, S, after);
}

// What every 12-lane pairing kernel starts with, after its LDS array
// (kSig12LdsWords words): its priority and kPad's padding, the wave's five
// teams on layout T (F: its register
// file) and the check each runs, idx (valid: idx < n; a padding team reads the
// inputs of the last check, ci). Out-parameters, not a struct: returning one
// moved the kernels' machine code.
static constexpr int kSig12LdsWords = kTeams12 * kSigTTeamElems * 10;
template <bool kPad>
HG_DEV Team sig12_team(uint32_t* lds, int n, uint32_t*& F, int& idx, bool& valid, int& ci) {
  // beside the GT fold on another stream: the pairing wave (the step's
  // critical path) wins the issue arbitration
  __builtin_amdgcn_s_setprio(3);
  // one pairing wave per SIMD: an allocation above half the VGPR file
  if constexpr (kPad) asm volatile("" ::: "v255", "a0");
  Team T = make_team12(lds, kSigTTeamElems * 10);
  F = T.base + kSigTRegBase * 10;
  idx = blockIdx.x * kTeams12 + team12_index();
  valid = idx < n;
  ci = valid ? idx : n - 1;
  return T;
}

// The final exponentiation's parking records (bn256_sigfe.h): res in fe[idx]
// (the result overwrites it), t0 in park[idx]; a padding team (idx >= n) uses
// the spare records park[n + 1 + (idx - n)] and park[n + 1 + kTeams12 +
// (idx - n)] (park has n + 1 + 2 kTeams12 records, Sig12Layout). Recomputed
// at each use.
struct Sig12Park {
  Gt *fe, *park;
  int n;
  HG_DEV uint32_t* operator()(int k) const {
    const int i = blockIdx.x * kTeams12 + team12_index();
    if (k == 0) return (i < n ? fe + i : park + n + 1 + (i - n))->w;
    return (i < n ? park + i : park + n + 1 + kTeams12 + (i - n))->w;
  }
};

// fe[r] = FE(Miller(G2Base at -sig_r)) on layout T (kSigTTeamElems elements
// per team: 18.4 KB of LDS per wave), five teams per wave. The final
// exponentiation parks two values per check in HBM: fe[r] itself (the result
// overwrites it) and park[r]. kPad: one pairing wave per SIMD (as
// k_verify_sig's default); unpadded, two batches' waves share a SIMD.
template <bool kPad>
__global__ __launch_bounds__(64, kPad ? 1 : 2) void k_verify_sig12(const Fp* ev, const Fp* sc, int n, Gt* fe,
                                                                   Gt* park) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<kPad>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  team_miller_sig12(T, F, ev, sc, n, ci, S, SigFE<SigProgs12>::final_exp_hint_t());
  SigFE<SigProgs12>::team_final_exp_fc_t(T, S, Sig12Park{fe, park, n});
  team_sync();
  Fp v;
  ld_fp_a8(v, slot(T, S_F) + T.e * 10);
  if (valid && T.active) {
    uint2* dst = (uint2*)__builtin_assume_aligned(fe[idx].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
}

// ---------------------------------------------------------------- split form
// The same chain in three kernels, so that the one Fp inversion per check
// (the norm of f down to Fp, t12_inv_norm's Bernstein-Yang inversion: 4.3 %
// of k_verify_sig12's VALU instructions and 13 % of its SALU ones, measured
// by dropping it, profiles/r06p_inv_probe.json) is done for 256 checks at
// a time instead of once per wave:
//   k_sig12_miller  the Miller loop and the norm N = f conj(f) (bn256_sigfe.h
//                   fe_t_norm), then t12_inv_norm up to d (t12_inv_norm_terms):
//                   f -> fe[c], the terms -> hand[c], n = |d|^2 -> nrm[c]
//   k_sig12_ninv    nrm[c]^-1 for every check, by a product tree per 256
//                   checks and ONE inversion at its root
//   k_sig12_fe      f back into the team region, N^-1 from the terms and
//                   n^-1 (t12_inv_norm_finish), the rest of the chain
// The values are the monolithic kernel's, bit for bit: n^-1 is the unique
// canonical inverse either way, and every other operation is the same.
struct SigHand {
  Fp v[8];  // t0, t1, t2, d (x, y each)
};

// lane tl < 8 stores term value tl, lane 8 the norm (team-uniform values)
HG_DEV void sig12_store_terms(const Team& T, bool valid, const NormTerms& o, const Fp& nr, SigHand* hand, Fp* nrm) {
  if (valid && T.tl < 9) {
    Fp2 pick;  // (selects on values, not on member references: no scratch)
    f2_sel(pick, T.tl < 6, o.t2, o.d);
    f2_sel(pick, T.tl < 4, o.t1, pick);
    f2_sel(pick, T.tl < 2, o.t0, pick);
    Fp w;
    fp_sel(w, (T.tl & 1) == 0, pick.x, pick.y);
    fp_sel(w, T.tl == 8, nr, w);
    uint2* dst = (uint2*)__builtin_assume_aligned(T.tl == 8 ? nrm->l : hand->v[T.tl].l, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(w.l[2 * i], w.l[2 * i + 1]);
  }
}

template <bool kPad>
__global__ __launch_bounds__(64, kPad ? 1 : 2) void k_sig12_miller(const Fp* ev, const Fp* sc, int n, Gt* fe,
                                                                   SigHand* hand, Fp* nrm) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<kPad>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  team_miller_sig12(T, F, ev, sc, n, ci, S, xh<ISqr12T>());
  SigFE<SigProgs12>::fe_t_norm(T, S, xh_none());
  NormTerms o;
  Fp nr;
  t12_inv_norm_terms(T, S_B, o, nr);
  Fp v;
  ld_fp_a8(v, slot(T, S_F) + T.e * 10);
  if (valid && T.active) {
    uint2* dst = (uint2*)__builtin_assume_aligned(fe[idx].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
  sig12_store_terms(T, valid, o, nr, hand + idx, nrm + idx);
}

// f = fe[c] into slot F of layout T, with the registers the programs read
HG_DEV void sig12_load_f(const Team& T, uint32_t* F, const Gt* fe, int ci) {
  if (T.tl == 0) {
    Fp zero, one;
    fp_zero(zero);
    fp_one(one);
    st_fp(F + R_ZERO * 10, zero);
    st_fp(F + R_ONE * 10, one);
  }
  const uint2* src = (const uint2*)__builtin_assume_aligned(fe[ci].w + 10 * T.e, 8);
  uint32_t v[10];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint2 x = src[i];
    v[2 * i] = x.x;
    v[2 * i + 1] = x.y;
  }
  if (T.active) st_fp_a8(slot(T, S_F) + T.e * 10, v);
  team_sync();
}

// k_sig12_miller's second half for a Miller value computed elsewhere (config
// 2's k_verify_ml, bn256_verify.hip): f = fe[c], the norm N = f conj(f)
// (fe_t_norm), then t12_inv_norm up to d: the terms -> hand[c], n -> nrm[c]
__global__ __launch_bounds__(64, 2) void k_sig12_norm(int n, const Gt* fe, SigHand* hand, Fp* nrm) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<false>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  sig12_load_f(T, F, fe, ci);
  SigFE<SigProgs12>::fe_t_norm(T, S, xh_none());
  NormTerms o;
  Fp nr;
  t12_inv_norm_terms(T, S_B, o, nr);
  sig12_store_terms(T, valid, o, nr, hand + idx, nrm + idx);
}

// ninv[c] = nrm[c]^-1, and 0 for 0. A sig-side Miller value is never zero
// (its lines all have the coefficient 1 at w^3, so f and its norms are
// nonzero), but config 2's split form sends the pk-side values of
// k_verify_ml through k_sig12_norm, and a go-flavor pk of order 13 on the
// twist has the Miller value 0 (the reference's too: its GT bytes are 384
// zeros). So the zero guard is live: without it one such key would zero the
// root and turn the other 255 checks of its block invalid
// (tests/test_gpu_small_order_keys.py). Per block of 256 checks:
// a product tree in LDS (8 levels), one fp_inv at the root, the inverses
// back down (inv(left) = inv(parent) right, inv(right) = inv(parent) left).
static constexpr int kInvBlock = 256;
__global__ __launch_bounds__(kInvBlock) void k_sig12_ninv(const Fp* nrm, int n, Fp* ninv) {
  // levels of the tree: the 256 leaves at 0, then 128 nodes at 256, 64 at
  // 384, ..., the root at 510
  __shared__ Fp tree[2 * kInvBlock];
  const int t = threadIdx.x;
  const int c = blockIdx.x * kInvBlock + t;
  Fp x, one;
  fp_one(one);
  x = one;
  const bool use = c < n && !fp_is_zero(nrm[c]);
  if (use) x = nrm[c];
  tree[t] = x;
  __syncthreads();
  int off = 0;  // the level of 2 sz nodes being multiplied pairwise
  for (int sz = kInvBlock / 2; sz >= 1; sz >>= 1) {
    if (t < sz) fp_mul(tree[off + 2 * sz + t], tree[off + 2 * t], tree[off + 2 * t + 1]);
    off += 2 * sz;
    __syncthreads();
  }
  // off: the root's index
  if (t == 0) fp_inv(tree[off], tree[off]);
  __syncthreads();
  for (int sz = 1; sz <= kInvBlock / 2; sz <<= 1) {  // down: the 2 sz children of the level of sz nodes at off
    const int child = off - 2 * sz;
    Fp pinv, sib;
    if (t < 2 * sz) {
      pinv = tree[off + (t >> 1)];
      sib = tree[child + (t ^ 1)];
    }
    __syncthreads();
    if (t < 2 * sz) fp_mul(tree[child + t], pinv, sib);
    off = child;
    __syncthreads();
  }
  if (c < n) {
    Fp z;
    fp_zero(z);
    fp_sel(x, use, tree[t], z);
    ninv[c] = x;
  }
}

template <bool kPad>
__global__ __launch_bounds__(64, kPad ? 1 : 2) void k_sig12_fe(int n, Gt* fe, Gt* park, const SigHand* hand,
                                                               const Fp* ninv) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<kPad>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  sig12_load_f(T, F, fe, ci);  // the registers the programs read, f into slot F
  t12_conj(T, S_D, S_F);
  NormTerms o;
  const SigHand& h = hand[ci];
  o.t0.x = h.v[0];
  o.t0.y = h.v[1];
  o.t1.x = h.v[2];
  o.t1.y = h.v[3];
  o.t2.x = h.v[4];
  o.t2.y = h.v[5];
  o.d.x = h.v[6];
  o.d.y = h.v[7];
  t12_inv_norm_finish(T, S_B, o, ninv[ci]);
  SigFE<SigProgs12>::fe_t_rest(T, S, Sig12Park{fe, park, n});
  team_sync();
  Fp v;
  ld_fp_a8(v, slot(T, S_F) + T.e * 10);
  if (valid && T.active) {
    uint2* dst = (uint2*)__builtin_assume_aligned(fe[idx].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
}

// One workspace layout for both callers: [the evaluated lines] | the parking
// records | [the signatures' scalars] | the split form's hand-over records |
// norms | inverses, each 256-byte aligned. lines: the bracketed members of a
// pairing from signatures (launch_sig12); config 2's final exponentiation of
// given Miller values (launch_fe12) has neither.
struct Sig12Layout {
  size_t park, scalars, hand, norm, ninv, bytes;
  Sig12Layout(int n, bool lines) {
    auto align256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    park = lines ? align256((size_t)n * kNumLines * 4 * sizeof(Fp)) : 0;
    scalars = park + align256((size_t)(n + 1 + 2 * kTeams12) * sizeof(Gt));
    hand = scalars + (lines ? align256((size_t)n * kSigScalars * sizeof(Fp)) : 0);
    norm = hand + align256((size_t)n * sizeof(SigHand));
    ninv = norm + align256((size_t)n * sizeof(Fp));
    bytes = ninv + (size_t)n * sizeof(Fp);
  }
};
size_t sig12_lines_bytes(int n) { return Sig12Layout(n, true).bytes; }
size_t fe12_ws_bytes(int n) { return Sig12Layout(n, false).bytes; }

// The split chain on workspace `base` laid out by L: the first kernel is
// k_sig12_miller from the evaluated lines ev, or (ev == nullptr) k_sig12_norm
// of the Miller values already in fe; then the batched inversion and the rest
// of the final exponentiation, in place.
static void launch_split_chain(const Fp* ev, int n, Gt* fe, uint8_t* base, const Sig12Layout& L, hipStream_t s) {
  const Fp* sc = (const Fp*)(base + L.scalars);
  Gt* park = (Gt*)(base + L.park);
  SigHand* hand = (SigHand*)(base + L.hand);
  Fp* nrm = (Fp*)(base + L.norm);
  Fp* ninv = (Fp*)(base + L.ninv);
  const int blocks = (n + kTeams12 - 1) / kTeams12;
  if (ev) k_sig12_miller<false><<<blocks, 64, 0, s>>>(ev, sc, n, fe, hand, nrm);
  else k_sig12_norm<<<blocks, 64, 0, s>>>(n, fe, hand, nrm);
  k_sig12_ninv<<<(n + kInvBlock - 1) / kInvBlock, kInvBlock, 0, s>>>(nrm, n, ninv);
  k_sig12_fe<false><<<blocks, 64, 0, s>>>(n, fe, park, hand, ninv);
}

// The launchers below refuse (false, nothing launched) a batch above
// kSig12MaxN: k_sig_lines indexes 4 n threads in int. sig_form() and
// verify_split_for() (bn256_sigform.h) never choose these forms there; a
// caller that got here anyway must not leave its codes at HG_OK.
bool launch_fe12(Gt* fe, int n, uint8_t* ws, hipStream_t s) {
  if (n > kSig12MaxN) return false;
  if (n > 0) launch_split_chain(nullptr, n, fe, ws, Sig12Layout(n, false), s);
  return true;
}

// launch_sig_form's T12Pad (pad) and T12 (split: sig_form_split) bodies
bool launch_sig12(bool pad, bool split, const uint8_t* sigs, int flavor, int n, const LineCoef* tab, uint8_t* ws,
                  Gt* fe, hipStream_t s) {
  if (n > kSig12MaxN) return false;
  if (n <= 0) return true;
  const Sig12Layout L(n, true);
  Fp* ev = (Fp*)ws;
  Fp* sc = (Fp*)(ws + L.scalars);
  k_sig_scalars<<<(n + kLineBlock - 1) / kLineBlock, kLineBlock, 0, s>>>(sigs, flavor, n, sc);
  k_sig_lines<<<dim3((4 * n + kLineBlock - 1) / kLineBlock, kNumLines), kLineBlock, 0, s>>>(sc, n, tab, ev);
  const int blocks = (n + kTeams12 - 1) / kTeams12;
  Gt* park = (Gt*)(ws + L.park);
  if (split) launch_split_chain(ev, n, fe, ws, L, s);
  else if (pad) k_verify_sig12<true><<<blocks, 64, 0, s>>>(ev, sc, n, fe, park);
  else k_verify_sig12<false><<<blocks, 64, 0, s>>>(ev, sc, n, fe, park);
  return true;
}

}  // namespace hg
