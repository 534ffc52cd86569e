// bn256_msgsrlc.hip — one final exponentiation for a group of aggregate checks
// that each carry their own message (hg_verify_aggregate_msgs_rlc,
// host side in hg_msgs_rlc.cpp). For the live requests i of a group, with
// secret 64-bit coefficients r_i,
//     prod e(r_i H_i, agg_i) * e(-sum r_i sig_i, G2Base) == 1
// holds when every check of the group holds (processing.go:342-368
// verifySignature, crypto.go:120-137 VerifyMultiSignature with msg per call),
// and otherwise with probability <= 2^-64: every e(H_i, agg_i) e(-sig_i, G2Base)
// lies in the order-n subgroup when the registry is proven in G2. A request
// costs one Miller loop and one Fp12 product, a group one final exponentiation.
//   k_mrlc_scalars  r_i k_i mod Order, one thread per request: the existing
//                   fixed-base kernel (k_hash_points) then gives r_i H_i
//   k_mrlc_sigs     the decoded signatures out of the check records, for the
//                   G1 kernels of bn256_rlc.hip (k_rlc_g1_mul, k_rlc_g1_sum)
//   k_mrlc_carrier  the first live member of every group
//   k_mrlc_checks   the scaled check records: agg_i, and the group's G1 sum on
//                   the carrier alone. The joint Miller loop multiplies the
//                   G2Base lines into every check; for a signature at infinity
//                   they are w^3, which the final exponentiation maps to one,
//                   so the group's signature-side loop rides in one member's.
//   k_mrlc_miller   k_verify_ml<4>'s body on hpts[check] (layout V), f_i stored
//   k_mrlc_product  the group's product of f_i over its live members: five
//                   12-lane teams a wave, one wave per group (FOLD region)
//   k_mrlc_gather   the failed groups' live members into compact arrays for
//                   the exact recheck (k_msgs_verify), in index order, ranked
//                   by bn256_rlc.hip's per-block counts (launch_rlc_failed_scan)
#include <hip/hip_runtime.h>

#include "bn256_gt.h"
#include "bn256_gtfold.h"
#include "bn256_mrlc.h"
#include "bn256_rlc.h"
#include "bn256_sigpair.h"

namespace hg {

__global__ __launch_bounds__(64) void k_mrlc_scalars(const uint32_t* k, const int32_t* hcodes, const uint64_t* r, int n,
                                                     uint32_t* rk) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = 0;
  if (hcodes[i] == HG_OK) {
    const uint4* src = (const uint4*)(k + 8 * (size_t)i);
    const uint4 lo = src[0], hi = src[1];
    const uint32_t kw[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    mrlc_scale(w, r[i], kw);
  }
  uint4* dst = (uint4*)(rk + 8 * (size_t)i);
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(256) void k_mrlc_sigs(const CheckIn* in, int n, PointG1* pts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) pts[i] = in[i].sig;
}

// one wave per group: carrier[g] = its first member whose code is HG_OK (none: 0xffffffff)
__global__ __launch_bounds__(64) void k_mrlc_carrier(const int32_t* codes, int n, uint32_t group, uint32_t* carrier) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const size_t base = (size_t)g * group;
  const int cnt = (int)min((size_t)group, (size_t)n - base);
  uint32_t first = 0xffffffffu;
#pragma unroll 1
  for (int blk = 0; blk < cnt; blk += 64) {  // wave-uniform
    const uint64_t bal = __ballot(blk + lane < cnt && codes[base + blk + lane] == HG_OK);
    if (bal == 0) continue;
    first = (uint32_t)(base + blk) + (uint32_t)(__ffsll((unsigned long long)bal) - 1);
    break;
  }
  if (lane == 0) carrier[g] = first;
}

__global__ __launch_bounds__(64) void k_mrlc_checks(const CheckIn* in, const int32_t* codes, const PointG1* gpts,
                                                    const uint32_t* carrier, int n, uint32_t group, CheckIn* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = (uint32_t)i / group;
  const bool live = codes[i] == HG_OK;
  PointG2 pk = in[i].pk;
  if (!live) pk.inf = 1;
  PointG1 sig;
  fp_zero(sig.x);
  fp_zero(sig.y);
  sig.inf = 1;
  sig.pad[0] = sig.pad[1] = sig.pad[2] = 0;
  if (live && carrier[g] == (uint32_t)i) sig = gpts[g];
  out[i].pk = pk;
  out[i].sig = sig;
}

// k_verify_ml<4> (bn256_verify.hip: layout V, the Miller value stored) with the
// check's own H, as k_msgs_miller (bn256_msgs.hip)
__global__ __launch_bounds__(64) void k_mrlc_miller(const CheckIn* in, int n, const LineCoef* tab,
                                                    const PointG1* hpts, Gt* fe) {
  constexpr int TEAMS = kTeamsPerBlock;
  constexpr int kWords = kVTeamElems * 10;
  __shared__ __attribute__((aligned(16))) uint32_t lds[TEAMS * kWords];
  Team T = make_team(lds, kWords);
  uint32_t* F = T.base + kVRegBase * 10;
  const int idx = blockIdx.x * TEAMS + (threadIdx.x >> 4);
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;
  const CheckIn& I = in[ci];
  const CheckCtx C = check_ctx(I, hpts + ci);
  XStream S = x_stream();
  team_miller_check<MillerV>(T, F, C, tab, true, S, xh_none());
  Fp v;
  ld_fp(v, slot(T, S_F) + T.e * 10);
  if (valid && T.active) {
    uint2* dst = (uint2*)__builtin_assume_aligned(fe[idx].w + 10 * T.e, 8);
#pragma unroll
    for (int i = 0; i < 5; i++) dst[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
  }
}

// One wave per group. The wave reads 64 members' codes at a time; a ballot per
// team gives team t the live members t, t + 5, ... of the group, and every team
// walks its own mask with the next value in flight across the product (as
// k_rlc_subsets, bn256_rlc.hip); a team whose mask runs out before the wave's
// longest multiplies by one. Then team 0 multiplies the other teams' partial
// products into its own (they multiply by one meanwhile, which leaves their
// value as it is): at most ceil(group / 5) + 4 products in a row.
__global__ __launch_bounds__(64) void k_mrlc_product(const Gt* f, const int32_t* codes, int n, uint32_t group,
                                                     Gt* z) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);
  fold_regs_init(T);
  const int team = team12_index(), lane = threadIdx.x;
  const int g = blockIdx.x;
  const size_t base = (size_t)g * group;
  const int cnt = (int)min((size_t)group, (size_t)n - base);
  XStream S = x_stream();
  Fp one;
  gt_one_value(one, T);
  gt_put(T, S_A, one, false);
#pragma unroll 1
  for (int blk = 0; blk < cnt; blk += 64) {  // wave-uniform
    const size_t first = base + blk;
    const bool live = blk + lane < cnt && codes[first + lane] == HG_OK;
    const int mine = (blk + lane) % kTeams12;
    uint64_t m = 0;
#pragma unroll
    for (int t = 0; t < kTeams12; t++) {
      const uint64_t bal = __ballot(live && mine == t);
      if (team == t) m = bal;
    }
    int rounds = __popcll(m);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) rounds = max(rounds, __shfl_xor(rounds, d));
    Fp nx = one;
    bool have = m != 0;
    if (have) {
      gt_read(nx, f + first + (__ffsll((unsigned long long)m) - 1), T);
      m &= m - 1;
    }
#pragma unroll 1
    for (int k = 0; k < rounds; k++) {
      Fp v;
      fp_sel(v, have, nx, one);
      gt_put(T, S_B, v, false);
      have = m != 0;
      if (have) {
        gt_read(nx, f + first + (__ffsll((unsigned long long)m) - 1), T);
        m &= m - 1;
      }
      fold_mul(T, S);
    }
  }
  const int a_off = (int)(slot(T, S_A) - T.base);
#pragma unroll 1
  for (int t = 1; t < kTeams12; t++) {
    team_sync();
    Fp v;
    ld_fp_a8(v, lds + t * kFoldWords + a_off + T.e * 10);
    fp_sel(v, team == 0, v, one);
    gt_put(T, S_B, v, false);
    fold_mul(T, S);
  }
  team_sync();
  if (team == 0) gt_store(T, S_A, z + g);
}

// ------------------------------------------------------------------ failed groups
__global__ __launch_bounds__(256) void k_mrlc_gather(const int32_t* codes, const int32_t* gcodes, int n,
                                                     uint32_t group, const CheckIn* in, const PointG1* h,
                                                     const uint32_t* bcount, uint32_t* idx, CheckIn* cchecks,
                                                     PointG1* ch, int32_t* ccodes) {
  __shared__ uint32_t wtot[4];
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const bool fl = rlc_failed_member(codes, gcodes, n, group, i);
  const uint64_t bal = __ballot(fl);
  const int wv = t >> 6, lane = t & 63;
  if (lane == 0) wtot[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (!fl) return;
  uint32_t j = bcount[blockIdx.x] + (uint32_t)__popcll(bal & (((uint64_t)1 << lane) - 1));
  for (int w = 0; w < wv; w++) j += wtot[w];
  idx[j] = (uint32_t)i;
  ccodes[j] = HG_OK;
  cchecks[j] = in[i];
  ch[j] = h[i];
}

// ------------------------------------------------------------------ launchers
void launch_mrlc_scalars(const uint32_t* k, const int32_t* hcodes, const uint64_t* r, int n, uint32_t* rk,
                         hipStream_t s) {
  if (n > 0) k_mrlc_scalars<<<nblk(n, 64), 64, 0, s>>>(k, hcodes, r, n, rk);
}
void launch_mrlc_sigs(const CheckIn* in, int n, PointG1* pts, hipStream_t s) {
  if (n > 0) k_mrlc_sigs<<<nblk(n, 256), 256, 0, s>>>(in, n, pts);
}
void launch_mrlc_checks(const CheckIn* in, const int32_t* codes, const PointG1* gpts, int n, uint32_t group,
                        int ngroups, uint32_t* carrier, CheckIn* out, hipStream_t s) {
  if (n <= 0) return;
  k_mrlc_carrier<<<ngroups, 64, 0, s>>>(codes, n, group, carrier);
  k_mrlc_checks<<<nblk(n, 64), 64, 0, s>>>(in, codes, gpts, carrier, n, group, out);
}
void launch_mrlc_miller(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, Gt* f, hipStream_t s) {
  if (n > 0) k_mrlc_miller<<<nblk(n, 4), 64, 0, s>>>(in, n, tab, hpts, f);
}
void launch_mrlc_product(const Gt* f, const int32_t* codes, int n, uint32_t group, int ngroups, Gt* z,
                         hipStream_t s) {
  if (n > 0) k_mrlc_product<<<ngroups, 64, 0, s>>>(f, codes, n, group, z);
}
void launch_mrlc_gather(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, const CheckIn* in,
                        const PointG1* h, uint32_t* bcount, uint32_t* idx, CheckIn* cchecks, PointG1* ch,
                        int32_t* ccodes, hipStream_t s) {
  if (n <= 0) return;
  launch_rlc_failed_scan(codes, gcodes, n, group, bcount, s);
  k_mrlc_gather<<<nblk(n, 256), 256, 0, s>>>(codes, gcodes, n, group, in, h, bcount, idx, cchecks, ch, ccodes);
}

}  // namespace hg
