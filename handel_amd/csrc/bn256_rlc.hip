// bn256_rlc.hip — one pairing for a group of aggregate checks (DESIGN.md §3l;
// hg_verify_aggregate_rlc, host side in hg_rlc.cpp). For the live checks i of
// a group, with secret 64-bit coefficients r_i,
//     e(sum r_i sig_i, G2Base) == prod F_i^(r_i),   F_i = e(H, aggregate key of i)
// holds when every check of the group holds (processing.go:342-368
// verifySignature, bn256/go/bn256.go:82-94), and otherwise with probability
// <= 2^-64. The GT fold already leaves X_i with F_i's conjugate = X_i (a
// classical table set) or X_i / conj(X_i) (a torus set). Here:
//   k_rlc_prep     the coefficients
//   k_rlc_g1_mul   r_i sig_i, one thread per check (64-bit double-and-add)
//   k_rlc_g1_sum   the group's sum over its live members, affine, and their count
//                  (one workgroup per group)
//   k_rlc_subsets  P_{g,b} = prod of X_i over the live i of group g with bit b
//                  of r_i set: one 12-lane team per (g, b), a chain of MUL12F
//                  as in the fold's chunk kernel (FOLD region, five teams a wave)
//   k_rlc_horner   Z_g = ((P_63)^2 P_62)^2 ... P_0 = prod X_i^(r_i): the 63
//                  squarings are shared by the whole group, so a group costs
//                  about 32 group + 126 products instead of 96 group
//   k_rlc_count, k_rlc_bcount, k_rlc_scan, k_rlc_gather, k_rlc_scatter
//                  the failed groups' live members into compact arrays for the
//                  exact recheck, in index order, and its codes back
// Conjugation is a ring automorphism, so prod (X_i / conj X_i)^(r_i) =
// Z_g / conj(Z_g): the existing comparisons take Z_g as they take a fold value.
#include <hip/hip_runtime.h>

#include "bn256_gt.h"
#include "bn256_gtfold.h"
#include "bn256_rlc.h"

namespace hg {

__global__ __launch_bounds__(256) void k_rlc_prep(RlcSeed seed, const uint64_t* coeffs, int n, uint64_t* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  r[i] = coeffs ? coeffs[i] : rlc_coeff(seed.b, (uint64_t)i);
}

// ------------------------------------------------------------------ the G1 side
// (codes may be read while the fold marks empty aggregates: either value serves,
// the sum goes by the codes the fold leaves)
__global__ __launch_bounds__(64) void k_rlc_g1_mul(const PointG1* pts, const int32_t* codes, const uint64_t* r, int n,
                                                   RlcJac* jac) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1J acc;
  g1_set_inf(acc);
  const PointG1 P = pts[i];
  if (codes[i] == HG_OK && !P.inf) {
    const uint64_t k = r[i];
#pragma unroll 1
    for (int bit = 63; bit >= 0; bit--) {
      g1_double(acc, acc);
      if ((k >> bit) & 1) g1_madd(acc, acc, P.x, P.y);
    }
  }
  RlcJac o;
  o.x = acc.x;
  o.y = acc.y;
  o.z = acc.z;
  jac[i] = o;
}

// The sum over the group's live members (codes: as they are after the fold; the
// multiples were taken on the prologue's codes, beside the fold) and their
// count. g1_add's own handling of equal inputs (doubling), opposite inputs and
// infinity makes the sum the exact group element whatever the members are.
__global__ __launch_bounds__(64) void k_rlc_g1_sum(const RlcJac* jac, const int32_t* codes, int n, uint32_t group,
                                                   PointG1* gpts, uint32_t* glive) {
  __shared__ RlcJac sh[64];
  const int g = blockIdx.x, t = threadIdx.x;
  const size_t base = (size_t)g * group;
  const int cnt = (int)min((size_t)group, (size_t)n - base);
  G1J acc;
  g1_set_inf(acc);
  int live = 0;
#pragma unroll 1
  for (int j = t; j < cnt; j += 64) {
    if (codes[base + j] != HG_OK) continue;
    live++;
    const RlcJac m = jac[base + j];
    G1J b;
    b.x = m.x;
    b.y = m.y;
    b.z = m.z;
    g1_add(acc, acc, b);
  }
#pragma unroll 1
  for (int d = 32; d > 0; d >>= 1) {
    RlcJac o;
    o.x = acc.x;
    o.y = acc.y;
    o.z = acc.z;
    sh[t] = o;
    __syncthreads();
    if (t < d) {
      const RlcJac m = sh[t + d];
      G1J b;
      b.x = m.x;
      b.y = m.y;
      b.z = m.z;
      g1_add(acc, acc, b);
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) live += __shfl_xor(live, d);
  if (t == 0) {
    glive[g] = (uint32_t)live;
    PointG1 P;
    P.pad[0] = P.pad[1] = P.pad[2] = 0;
    if (g1_is_inf(acc)) {
      fp_zero(P.x);
      fp_zero(P.y);
      P.inf = 1;
    } else {
      g1_affine(P.x, P.y, acc);
      P.inf = 0;
    }
    gpts[g] = P;
  }
}

// ------------------------------------------------------------------ the GT side
// Stage 1. A workgroup (one wave, five teams) takes five bits of one group: the
// wave reads 64 members' coefficients at a time (0 for a member that is not
// live), a ballot per bit gives each team its members, and every team walks
// its own mask, so a team multiplies only by members that have its bit; a team
// whose mask runs out before the wave's longest multiplies by one.
static constexpr int kRlcWavesPerGroup = (kRlcBits + kTeams12 - 1) / kTeams12;
__global__ __launch_bounds__(64) void k_rlc_subsets(const Gt* x, const int32_t* codes, const uint64_t* r, int n,
                                                    uint32_t group, Gt* P) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);
  fold_regs_init(T);
  const int team = team12_index(), lane = threadIdx.x;
  const int g = blockIdx.x / kRlcWavesPerGroup, bit0 = (blockIdx.x % kRlcWavesPerGroup) * kTeams12;
  const int bit = bit0 + team;
  const size_t base = (size_t)g * group;
  const int cnt = (int)min((size_t)group, (size_t)n - base);
  XStream S = x_stream();
  Fp one;
  gt_one_value(one, T);
  gt_put(T, S_A, one, false);
#pragma unroll 1
  for (int blk = 0; blk < cnt; blk += 64) {  // wave-uniform
    const size_t first = base + blk;
    uint64_t rr = 0;
    if (blk + lane < cnt && codes[first + lane] == HG_OK) rr = r[first + lane];
    uint64_t m = 0;
#pragma unroll
    for (int t = 0; t < kTeams12; t++) {
      const int b = bit0 + t;
      const uint64_t bal = __ballot(b < kRlcBits && ((rr >> (b & 63)) & 1));
      if (team == t) m = bal;
    }
    int rounds = __popcll(m);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) rounds = max(rounds, __shfl_xor(rounds, d));
    // the next member's value in flight across the product
    Fp nx = one;
    bool have = m != 0;
    if (have) {
      gt_read(nx, x + first + (__ffsll((unsigned long long)m) - 1), T);
      m &= m - 1;
    }
#pragma unroll 1
    for (int k = 0; k < rounds; k++) {
      Fp v;
      fp_sel(v, have, nx, one);
      gt_put(T, S_B, v, false);
      have = m != 0;
      if (have) {
        gt_read(nx, x + first + (__ffsll((unsigned long long)m) - 1), T);
        m &= m - 1;
      }
      fold_mul(T, S);
    }
  }
  team_sync();
  if (bit < kRlcBits && T.active) gt_store(T, S_A, P + (size_t)g * kRlcBits + bit);
}

// Stage 2. One team per group, five groups a wave: 63 squarings and 63 products,
// the same count for every group, so the wave's teams stay in step.
__global__ __launch_bounds__(64) void k_rlc_horner(const Gt* P, int ngroups, Gt* z) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTeams12 * kFoldWords];
  Team T = make_team12(lds, kFoldWords);
  fold_regs_init(T);
  const int g = blockIdx.x * kTeams12 + team12_index();
  const Gt* p = P + (size_t)min(g, ngroups - 1) * kRlcBits;
  XStream S = x_stream();
  gt_load(T, S_A, p + kRlcBits - 1);
  Fp nx;
  gt_read(nx, p + kRlcBits - 2, T);
#pragma unroll 1
  for (int b = kRlcBits - 2; b >= 0; b--) {
    team_sync();
    lds_fp12_copy(T, slot(T, S_B), slot(T, S_A));
    fold_mul(T, S);  // A = A^2
    team_sync();
    gt_put(T, S_B, nx, false);
    if (b > 0) gt_read(nx, p + b - 1, T);
    fold_mul(T, S);  // A = A P_b
  }
  team_sync();
  if (g < ngroups && T.active) gt_store(T, S_A, z + g);
}

// ------------------------------------------------------------------ failed groups
__global__ __launch_bounds__(256) void k_rlc_count(const int32_t* gcodes, const uint32_t* glive, int ngroups,
                                                   RlcHdr* hdr) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t live = glive[g];
  if (live == 0) return;
  atomicAdd(&hdr->groups, 1u);
  if (gcodes[g] != HG_OK) {
    atomicAdd(&hdr->groups_failed, 1u);
    atomicAdd(&hdr->failed_members, live);
  }
}
__global__ __launch_bounds__(256) void k_rlc_bcount(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group,
                                                    uint32_t* bcount) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c = __syncthreads_count(rlc_failed_member(codes, gcodes, n, group, i) ? 1 : 0);
  if (threadIdx.x == 0) bcount[blockIdx.x] = (uint32_t)c;
}
// exclusive prefix sum of bcount[0 .. nb) in place, one workgroup
__global__ __launch_bounds__(256) void k_rlc_scan(uint32_t* bcount, int nb) {
  __shared__ uint32_t sh[256];
  __shared__ uint32_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 256) {
    const uint32_t v = base + t < nb ? bcount[base + t] : 0u;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t a = t >= d ? sh[t - d] : 0u;
      __syncthreads();
      sh[t] += a;
      __syncthreads();
    }
    if (base + t < nb) bcount[base + t] = carry + sh[t] - v;
    __syncthreads();
    if (t == 0) carry += sh[255];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_rlc_gather(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group,
                                                    const uint8_t* sigs, const Gt* y, const uint32_t* bcount,
                                                    uint32_t* idx, uint8_t* csigs, Gt* cy, int32_t* ccodes) {
  __shared__ uint32_t wtot[4];
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const bool f = rlc_failed_member(codes, gcodes, n, group, i);
  const uint64_t bal = __ballot(f);
  const int wv = t >> 6, lane = t & 63;
  if (lane == 0) wtot[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (!f) return;
  uint32_t j = bcount[blockIdx.x] + (uint32_t)__popcll(bal & (((uint64_t)1 << lane) - 1));
  for (int w = 0; w < wv; w++) j += wtot[w];
  idx[j] = (uint32_t)i;
  ccodes[j] = HG_OK;
  for (int k = 0; k < 64; k++) csigs[(size_t)j * 64 + k] = sigs[(size_t)i * 64 + k];
  for (int k = 0; k < 120; k++) cy[j].w[k] = y[i].w[k];
}
__global__ __launch_bounds__(256) void k_rlc_scatter(const uint32_t* idx, const int32_t* ccodes, int m, int32_t* codes) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) codes[idx[j]] = ccodes[j];
}

// ------------------------------------------------------------------ launchers
void launch_rlc_prep(RlcSeed seed, const uint64_t* coeffs, int n, int ngroups, uint64_t* r, int32_t* gcodes,
                     RlcHdr* hdr, hipStream_t s) {
  if (n <= 0) return;
  (void)hipMemsetAsync(gcodes, 0, (size_t)ngroups * sizeof(int32_t), s);  // HG_OK
  (void)hipMemsetAsync(hdr, 0, sizeof(RlcHdr), s);
  k_rlc_prep<<<nblk(n, 256), 256, 0, s>>>(seed, coeffs, n, r);
}
void launch_rlc_g1_mul(const PointG1* pts, const int32_t* codes, const uint64_t* r, int n, RlcJac* jac, hipStream_t s) {
  if (n > 0) k_rlc_g1_mul<<<nblk(n, 64), 64, 0, s>>>(pts, codes, r, n, jac);
}
void launch_rlc_g1_sum(const RlcJac* jac, const int32_t* codes, int n, uint32_t group, int ngroups, PointG1* gpts,
                       uint32_t* glive, hipStream_t s) {
  if (n > 0) k_rlc_g1_sum<<<ngroups, 64, 0, s>>>(jac, codes, n, group, gpts, glive);
}
void launch_rlc_gt(const Gt* x, const int32_t* codes, const uint64_t* r, int n, uint32_t group, int ngroups, Gt* P,
                   Gt* z, hipStream_t s) {
  if (n <= 0) return;
  k_rlc_subsets<<<ngroups * kRlcWavesPerGroup, 64, 0, s>>>(x, codes, r, n, group, P);
  k_rlc_horner<<<nblk(ngroups, kTeams12), 64, 0, s>>>(P, ngroups, z);
}
void launch_rlc_count(const int32_t* gcodes, const uint32_t* glive, int ngroups, RlcHdr* hdr, hipStream_t s) {
  if (ngroups > 0) k_rlc_count<<<nblk(ngroups, 256), 256, 0, s>>>(gcodes, glive, ngroups, hdr);
}
void launch_rlc_failed_scan(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, uint32_t* bcount,
                            hipStream_t s) {
  if (n <= 0) return;
  const int nb = nblk(n, 256);
  k_rlc_bcount<<<nb, 256, 0, s>>>(codes, gcodes, n, group, bcount);
  k_rlc_scan<<<1, 256, 0, s>>>(bcount, nb);
}
void launch_rlc_gather(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, const uint8_t* sigs,
                       const Gt* y, uint32_t* bcount, uint32_t* idx, uint8_t* csigs, Gt* cy, int32_t* ccodes,
                       hipStream_t s) {
  if (n <= 0) return;
  launch_rlc_failed_scan(codes, gcodes, n, group, bcount, s);
  k_rlc_gather<<<nblk(n, 256), 256, 0, s>>>(codes, gcodes, n, group, sigs, y, bcount, idx, csigs, cy, ccodes);
}
void launch_rlc_scatter(const uint32_t* idx, const int32_t* ccodes, int m, int32_t* codes, hipStream_t s) {
  if (m > 0) k_rlc_scatter<<<nblk(m, 256), 256, 0, s>>>(idx, ccodes, m, codes);
}

}  // namespace hg
