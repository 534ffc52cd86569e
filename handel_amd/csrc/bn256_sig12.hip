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
// Team region (layout T, tools/gen_g2_schedule.py): five Fp12 slots and the
// register file, 92 elements (kSigTTeamElems; 94 before the shared-operand
// squaring of r06) — the final exponentiation parks two of its seven live
// values in HBM (bn256_sigfe.h team_final_exp_fc_t) — so a wave of five teams
// takes 18.4 KB of LDS and a CU holds eight pairing waves (two per SIMD: the
// unpadded kernels' 193-212 VGPRs allow it) beside a fold
// workgroup.
//
// Values are identical to k_verify_sig's (the same Montgomery products in the
// same order, canonical), so the FE values, and every verdict, are too.
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

// the signature's evaluation scalars: sc[2c] = x_sig, sc[2c + 1] = -y_sig
// (both 0 at infinity: e(inf, G2Base) = 1, every line evaluates to w^3, which
// the final exponentiation maps to 1 — bn256_sigteam.h team_miller_sig). A
// signature that fails to decode gives meaningless lines: its FE value is
// never compared (its code is the decode error, k_agg_prologue).
__global__ __launch_bounds__(kLineBlock) void k_sig_scalars(const uint8_t* sig_bytes, int flavor, int n, Fp* sc) {
  const int c = blockIdx.x * kLineBlock + threadIdx.x;
  if (c >= n) return;
  PointG1 sg;
  (void)decode_g1_one(sig_bytes + (size_t)c * 64, flavor, sg);
  Fp nsy, z;
  fp_zero(z);
  fp_neg(nsy, sg.y);
  const bool use = sg.inf == 0;
  fp_sel(sc[2 * c], use, sg.x, z);
  fp_sel(sc[2 * c + 1], use, nsy, z);
}

// ev[(s * n + c) * 4 + j] = component j of line s at -sig_c: one Montgomery
// product per thread (FB = bx * x_sig, FC = cy * -y_sig); grid (4n / 256,
// lines), consecutive threads on consecutive 40-byte results
__global__ __launch_bounds__(kLineBlock) void k_sig_lines(const Fp* sc, int n, const LineCoef* tab, Fp* ev) {
  const int t = blockIdx.x * kLineBlock + threadIdx.x;  // 4 c + j
  if (t >= 4 * n) return;
  const int s = blockIdx.y;
  const int j = t & 3;
  const int c = t >> 2;
  const Fp a = reinterpret_cast<const Fp*>(&tab[s])[j];
  const Fp b = sc[2 * c + (j >> 1)];
  Fp o;
  fp_mul(o, a, b);
  st_fp_g8(ev[(size_t)s * 4 * n + t].l, o);
}

// The evaluated line reaches the team's registers FB, FC through one VGPR
// element per lane (lane tl < 4 holds Fp tl), read from HBM one publication
// ahead so the read's latency overlaps the rounds between.
struct EvPipe {
  Fp c;
};
HG_DEV void ev_fetch(const Team& T, EvPipe& P, const Fp* ev, int n, int ci, int s) {
  if (T.tl < 4) ld_fp_g8(P.c, ev[((size_t)s * n + ci) * 4 + T.tl].l);
}
// the held line into FB, FC, then line `next` into flight
HG_DEV void ev_publish(const Team& T, uint32_t* F, EvPipe& P, const Fp* ev, int n, int ci, int next) {
  if (T.tl < 4) st_fp_a8(F + (R_FB_x + T.tl) * 10, P.c.l);
  team_sync();
  if (next < kNumLines) ev_fetch(T, P, ev, n, ci, next);
}

using ISqr12T = XInst<XP_SQR12_12_T, S_F, S_F>;
using ILineT = XInst<XP_LINE_FIX_12_T, S_F, S_F>;

// Miller(G2Base at -sig) over the NAF of 6u + 2 (bn256_sigteam.h
// team_miller_sig's loop; the lines arrive evaluated): f^2, then f * line
// per digit (two lines on a nonzero digit), then the two Frobenius lines
HG_DEV void team_miller_sig12(const Team& T, uint32_t* F, const Fp* ev, int n, int ci, XStream& S, XHint after) {
  const int8_t naf[kNafLen] = HG_NAF;
  t12_set_one(T, S_F);
  if (T.tl == 0) {
    Fp zero, one;
    fp_zero(zero);
    fp_one(one);
    st_fp(F + R_ZERO * 10, zero);
    st_fp(F + R_ONE * 10, one);
  }
  team_sync();
  EvPipe P;
  fp_zero(P.c);
  ev_fetch(T, P, ev, n, ci, 0);
  int s = 0;
  for (int i = kNafLen - 1; i > 0; i--) {
    const int d = naf[i - 1];
    ev_publish(T, F, P, ev, n, ci, s + 1);  // line s, read by the product after f^2
    ISqr12T::run(T, S, xh<ILineT>());      // f^2 (f = 1 on the first digit)
    const XHint after_digit = i > 1 ? xh<ISqr12T>() : xh<ILineT>();
    if (d != 0) {
      ILineT::run(T, S, xh<ILineT>());
      ev_publish(T, F, P, ev, n, ci, s + 2);  // line s + 1 (the addition's)
      ILineT::run(T, S, after_digit);
      s += 2;
    } else {
      ILineT::run(T, S, after_digit);
      s += 1;
    }
  }
  // the two Frobenius lines
  ev_publish(T, F, P, ev, n, ci, s + 1);
  ILineT::run(T, S, xh<ILineT>());
  ev_publish(T, F, P, ev, n, ci, kNumLines);
  ILineT::run(T, S, after);
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
__global__ __launch_bounds__(64, kPad ? 1 : 2) void k_verify_sig12(const Fp* ev, int n, Gt* fe, Gt* park) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<kPad>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  team_miller_sig12(T, F, ev, n, ci, S, SigFE<SigProgs12>::final_exp_hint_t());
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
__global__ __launch_bounds__(64, kPad ? 1 : 2) void k_sig12_miller(const Fp* ev, int n, Gt* fe, SigHand* hand,
                                                                   Fp* nrm) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSig12LdsWords];
  uint32_t* F;
  int idx, ci;
  bool valid;
  Team T = sig12_team<kPad>(lds, n, F, idx, valid, ci);
  XStream S = x_stream();
  team_miller_sig12(T, F, ev, n, ci, S, xh<ISqr12T>());
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
    hand = scalars + (lines ? align256((size_t)n * 2 * sizeof(Fp)) : 0);
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
  Gt* park = (Gt*)(base + L.park);
  SigHand* hand = (SigHand*)(base + L.hand);
  Fp* nrm = (Fp*)(base + L.norm);
  Fp* ninv = (Fp*)(base + L.ninv);
  const int blocks = (n + kTeams12 - 1) / kTeams12;
  if (ev) k_sig12_miller<false><<<blocks, 64, 0, s>>>(ev, n, fe, hand, nrm);
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
  else if (pad) k_verify_sig12<true><<<blocks, 64, 0, s>>>(ev, n, fe, park);
  else k_verify_sig12<false><<<blocks, 64, 0, s>>>(ev, n, fe, park);
  return true;
}

}  // namespace hg
