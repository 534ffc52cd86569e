// bn256_batchrlc.hip — one final exponentiation for a group of independent
// checks on arbitrary keys (hg_verify_batch_rlc,
// hg_verify_batch_msgs_rlc, host side in hg_batch_rlc.cpp). For the live checks
// i of a group, with secret 64-bit coefficients r_i,
//     prod e(r_i H_i, pk_i) * e(-sum r_i sig_i, G2Base) == 1
// holds when every check of the group holds (PublicKey.VerifySignature,
// bn256/go/bn256.go:82-94), and otherwise with probability <= 2^-64 provided
// every pk_i lies in G2: then every e(H_i, pk_i) e(-sig_i, G2Base) lies in the
// order-n subgroup. The keys are arbitrary twist points (x/crypto's
// G2.Unmarshal, bn256/go/bn256.go:113-120), so membership is decided here, by
// the Miller loop that runs anyway: it ends on
//     R = [6u+2]Q + psi(Q) - psi^2(Q),
// and R == -psi^3(Q) exactly when Q lies in G2 (proof in DESIGN §3n). The
// loop's step formulas are not complete; an exceptional step (R = +-addend, R at
// infinity, Y = 0) leaves W = 0 for good, so with Z = xi W and T = -psi^3(Q)
//     member(Q)  <=>  W != 0  and  X == T.x Z  and  Y == T.y Z.
// A group that holds a live check whose key is not a proven member fails,
// whatever its product, and its live members take the exact check.
//   k_brlc_one_message  the one-message form's per-check k, hcodes and H
//   k_brlc_miller       k_mrlc_miller's body, then the rule: f_i and member[i]
//   k_brlc_members      the group's live non-members into its code and the count
//   k_brlc_probe_checks hg_debug_g2_member's check records
// Everything else is bn256_msgsrlc.hip's and bn256_rlc.hip's.
#include <hip/hip_runtime.h>

#include "bn256_brlc.h"
#include "bn256_gt.h"
#include "bn256_gtfold.h"
#include "bn256_sigpair.h"

namespace hg {

__global__ __launch_bounds__(256) void k_brlc_one_message(BrlcScalar k1, const PointG1* h1, int32_t code, int n,
                                                          uint32_t* k, int32_t* hcodes, PointG1* h) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint4* dst = (uint4*)(k + 8 * (size_t)i);
  dst[0] = make_uint4(k1.w[0], k1.w[1], k1.w[2], k1.w[3]);
  dst[1] = make_uint4(k1.w[4], k1.w[5], k1.w[6], k1.w[7]);
  hcodes[i] = code;
  h[i] = *h1;
}

// The membership rule on the team's register file after the loop's last
// addition (PADD_F2_3). The registers may be lazy (in [0, 2p)): a product by
// the Montgomery one makes each value canonical before it is compared.
// Team-uniform: every lane reads the same registers.
HG_DEV bool brlc_member(const uint32_t* F, const PointG2& Q) {
  const Fp2 c[2] = HG_PSI3;
  Fp one;
  fp_one(one);
  auto canon = [&](Fp2& r, int rx) {
    Fp t;
    ld_fp(t, F + rx * 10);
    fp_mul(r.x, t, one);
    ld_fp(t, F + (rx + 1) * 10);
    fp_mul(r.y, t, one);
  };
  Fp2 X, Y, W, Z, t, tx, ty;
  canon(X, R_X_x);
  canon(Y, R_Y_x);
  canon(W, R_Z_x);
  f2_mul_xi(Z, W);
  // T = -psi^3(Q) = (conj(Qx) psi3[0], -conj(Qy) psi3[1])
  f2_conj(t, Q.x);
  f2_mul(tx, t, c[0]);
  f2_conj(t, Q.y);
  f2_mul(ty, t, c[1]);
  f2_mul(tx, tx, Z);
  f2_mul(ty, ty, Z);
  f2_neg(ty, ty);
  return !f2_is_zero(W) && f2_eq(X, tx) && f2_eq(Y, ty);
}

// k_mrlc_miller (bn256_msgsrlc.hip: layout V, the check's own H, the Miller
// value stored) and the rule. hstride: 1, or 0 for one H for every check.
__global__ __launch_bounds__(64) void k_brlc_miller(const CheckIn* in, int n, const LineCoef* tab,
                                                    const PointG1* hpts, int hstride, Gt* fe, uint32_t* member) {
  constexpr int TEAMS = kTeamsPerBlock;
  constexpr int kWords = kVTeamElems * 10;
  __shared__ __attribute__((aligned(16))) uint32_t lds[TEAMS * kWords];
  Team T = make_team(lds, kWords);
  uint32_t* F = T.base + kVRegBase * 10;
  const int idx = blockIdx.x * TEAMS + (threadIdx.x >> 4);
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;
  const CheckIn& I = in[ci];
  const CheckCtx C = check_ctx(I, hpts + (size_t)ci * hstride);
  XStream S = x_stream();
  team_miller_check<MillerV>(T, F, C, tab, true, S, xh_none());
  team_sync();
  // a key at infinity is a member (its loop ran on a placeholder)
  const bool mem = brlc_member(F, I.pk) || I.pk.inf != 0;
  Fp v, z, one;
  ld_fp(v, slot(T, S_F) + T.e * 10);
  fp_zero(z);
  fp_one(one);
  fp_sel(z, T.e == 1, one, z);  // element e of the Fp12 one (t12_set_one)
  fp_sel(v, mem, v, z);
  if (valid && T.active) {
    uint2* dst = (uint2*)__builtin_assume_aligned(fe[idx].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
  if (valid && T.tl == 0) member[idx] = mem ? 1u : 0u;
}

// one wave per group
__global__ __launch_bounds__(64) void k_brlc_members(const int32_t* codes, const uint32_t* member, int n,
                                                     uint32_t group, int32_t* gcodes, RlcHdr* hdr) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const size_t base = (size_t)g * group;
  const int cnt = (int)min((size_t)group, (size_t)n - base);
  uint32_t bad = 0;
#pragma unroll 1
  for (int j = lane; j < cnt; j += 64)
    if (codes[base + j] == HG_OK && member[base + j] == 0) bad++;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) bad += __shfl_xor(bad, d);
  if (lane == 0 && bad) {
    gcodes[g] = HG_ERR_SIG_INVALID;
    atomicAdd(&hdr->non_g2, bad);
  }
}

__global__ __launch_bounds__(256) void k_brlc_probe_checks(const PointG2* pks, const int32_t* codes, int n,
                                                           CheckIn* out, PointG1* gen) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fp z, one, two;
  fp_zero(z);
  fp_one(one);
  if (i == 0) {  // G1 = (1, -2)
    fp_add(two, one, one);
    gen->x = one;
    fp_neg(gen->y, two);
    gen->inf = 0;
    gen->pad[0] = gen->pad[1] = gen->pad[2] = 0;
  }
  out[i].pk = pks[i];
  if (codes[i] != HG_OK) out[i].pk.inf = 1;
  out[i].sig.x = z;
  out[i].sig.y = z;
  out[i].sig.inf = 1;
  out[i].sig.pad[0] = out[i].sig.pad[1] = out[i].sig.pad[2] = 0;
}

// ------------------------------------------------------------------ launchers
void launch_brlc_one_message(BrlcScalar k1, const PointG1* h1, int32_t code, int n, uint32_t* k, int32_t* hcodes,
                             PointG1* h, hipStream_t s) {
  if (n > 0) k_brlc_one_message<<<nblk(n, 256), 256, 0, s>>>(k1, h1, code, n, k, hcodes, h);
}
void launch_brlc_miller(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int hstride, Gt* f,
                        uint32_t* member, hipStream_t s) {
  if (n > 0) k_brlc_miller<<<nblk(n, 4), 64, 0, s>>>(in, n, tab, hpts, hstride ? 1 : 0, f, member);
}
void launch_brlc_members(const int32_t* codes, const uint32_t* member, int n, uint32_t group, int ngroups,
                         int32_t* gcodes, RlcHdr* hdr, hipStream_t s) {
  if (n > 0) k_brlc_members<<<ngroups, 64, 0, s>>>(codes, member, n, group, gcodes, hdr);
}
void launch_brlc_probe_checks(const PointG2* pks, const int32_t* codes, int n, CheckIn* out, PointG1* gen,
                              hipStream_t s) {
  if (n > 0) k_brlc_probe_checks<<<nblk(n, 256), 256, 0, s>>>(pks, codes, n, out, gen);
}

}  // namespace hg
