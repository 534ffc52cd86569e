// bn256_msgs.hip — batches whose checks each carry their own message
// (PublicKey.VerifySignature(msg, sig), bn256/go/bn256.go:82-94, with msg per
// call): hashedMessage (bn256/go/bn256.go:210-218) for every check on the
// device, and the pairing check reading its H per check.
//
//   k_hash_scalars    SHA-256 and the crypto/rand.Int rule, one thread per message
//   k_g1_base_table   the fixed-base table d 16^j G1 (once per context, on first use)
//   k_hash_points     k G1 from the table, one 16-lane team per message
//   k_msgs_verify     k_verify<4>'s body on hpts[check]
//   k_msgs_miller     k_verify_ml<4>'s body on hpts[check] (the split form's first half)
#include <hip/hip_runtime.h>

#include "bn256_curve.h"
#include "bn256_pairing.h"
#include "bn256_sigpair.h"
#include "hg_sha256.h"

namespace hg {
static inline int nblk(int n, int b) { return (n + b - 1) / b; }

// ------------------------------------------------------------------ hashedMessage's scalar
// Message i is pool[off[i] .. off[i] + len[i]) (any alignment, any length). A
// range that leaves the pool is not read: HG_ERR_ARG for that check alone.
__global__ __launch_bounds__(64) void k_hash_scalars(const uint8_t* pool, uint64_t pool_len, const uint32_t* off,
                                                    const uint32_t* len, int n, uint32_t* k, int32_t* hcodes) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = off[i], l = len[i];
  uint32_t w[8];
  int32_t code;
  if ((uint64_t)o + l > pool_len) {
    code = HG_ERR_ARG;
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
  } else {
    uint32_t h[8];
    sha256_words(pool + o, l, h);
    code = hash_scalar_words(h, w) ? HG_OK : HG_ERR_HASH_EOF;
  }
  uint4* dst = (uint4*)(k + 8 * (size_t)i);
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  hcodes[i] = code;
}

// ------------------------------------------------------------------ the G1 base table
// tab[15 j + d - 1] = d 16^j G1 for the 64 4-bit windows j and the digits
// d = 1..15, affine: one thread per entry walks the double-and-add of the
// scalar d << 4j (k_hash_point's chain, 960 of them side by side) and inverts
// its own z. No entry is infinity: the group order is prime and above 15.
__global__ __launch_bounds__(64) void k_g1_base_table(PointG1* tab) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= kG1TabEntries) return;
  const int j = e / kG1TabDigits, d = e % kG1TabDigits + 1;
  uint32_t k[8];
#pragma unroll
  for (int w = 0; w < 8; w++) k[w] = w == (j >> 3) ? (uint32_t)d << (4 * (j & 7)) : 0u;
  G1J g, r;
  const Fp gx = HG_G1X, gy = HG_G1Y;
  g.x = gx;
  g.y = gy;
  fp_one(g.z);
  g1_mul(r, g, k);
  PointG1 P;
  g1_affine(P.x, P.y, r);
  P.inf = 0;
  P.pad[0] = P.pad[1] = P.pad[2] = 0;
  tab[e] = P;
}

// ------------------------------------------------------------------ k G1, 16 lanes per scalar
// Four messages per wave, one 16-lane row each. Lane l holds the scalar's bits
// [16 l, 16 l + 16): it adds the table entries of windows 4l .. 4l + 3 (mixed
// additions, zero digits skipped, infinity when all four are zero). The 16
// partial sums then meet in a 4-level butterfly of full Jacobian additions
// (g1_add with its doubling and infinity branches: two partial sums are
// equal or opposite points only when they differ by a multiple of Order as
// integers, which the branches serve all the same); every lane ends with the
// sum, lane 0 converts it to affine. The inversion stays on that lane: at one
// team per message the wave has nothing else to run beside it, and a separate
// pass would wait for the same chain after a round trip through memory.
// A check whose hash code is not HG_OK takes the scalar 1 without reading k:
// its point is the generator, a placeholder that is never verified against.
__global__ __launch_bounds__(64) void k_hash_points(const uint32_t* k, const int32_t* hcodes, int n,
                                                   const PointG1* tab, PointG1* out) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;
  const bool hashed = hcodes == nullptr || hcodes[ci] == HG_OK;
  uint32_t bits = l == 0 ? 1u : 0u;
  if (hashed) bits = (k[8 * (size_t)ci + (l >> 1)] >> (16 * (l & 1))) & 0xffffu;
  G1J acc;
  g1_set_inf(acc);
#pragma unroll 1
  for (int t = 0; t < 4; t++) {
    const uint32_t d = (bits >> (4 * t)) & 15u;
    if (d == 0) continue;
    const PointG1& P = tab[(4 * l + t) * kG1TabDigits + (int)d - 1];
    g1_madd(acc, acc, P.x, P.y);
  }
#pragma unroll 1
  for (int s = 1; s < 16; s <<= 1) {
    G1J q;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      q.x.l[i] = __shfl_xor(acc.x.l[i], s, 16);
      q.y.l[i] = __shfl_xor(acc.y.l[i], s, 16);
      q.z.l[i] = __shfl_xor(acc.z.l[i], s, 16);
    }
    g1_add(acc, acc, q);
  }
  if (!valid || l != 0) return;
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
  out[idx] = P;
}

// hashedMessage's error lands where the check is still HG_OK: the unmarshal
// errors of pk and sig come first (the reference parses before it verifies)
__global__ __launch_bounds__(256) void k_merge_hash_codes(const int32_t* hcodes, int n, int32_t* codes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && codes[i] == HG_OK) codes[i] = hcodes[i];
}

// ------------------------------------------------------------------ the pairing check on hpts[check]
// k_verify<4> (bn256_verify.hip) with the check's own H
__global__ __launch_bounds__(64) void k_msgs_verify(const CheckIn* in, int n, const LineCoef* tab,
                                                   const PointG1* hpts, int32_t* codes) {
  constexpr int TEAMS = kTeamsPerBlock;
  __shared__ __attribute__((aligned(16))) uint32_t lds[TEAMS * kTeamWords];
  Team T = make_team(lds, kTeamWords);
  uint32_t* F = team_regs(T);
  const int idx = blockIdx.x * TEAMS + (threadIdx.x >> 4);
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;
  const CheckIn& I = in[ci];
  const CheckCtx C = check_ctx(I, hpts + ci);
  XStream S = x_stream();
  team_miller_check(T, F, C, tab, true, S, final_exp_hint());
  team_final_exp_fc(T, F, S);  // FE^m == 1 <=> FE == 1
  const bool ok = t12_is_one(T, S_F);
  if (valid && T.tl == 0 && codes[idx] == HG_OK) codes[idx] = ok ? HG_OK : HG_ERR_SIG_INVALID;
}

// k_verify_ml<4> (bn256_verify.hip: layout V, the Miller value stored for
// launch_fe12) with the check's own H
__global__ __launch_bounds__(64) void k_msgs_miller(const CheckIn* in, int n, const LineCoef* tab,
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

// ------------------------------------------------------------------ launchers
void launch_g1_base_table(PointG1* tab, hipStream_t s) {
  k_g1_base_table<<<nblk(kG1TabEntries, 64), 64, 0, s>>>(tab);
}
void launch_hash_scalars(const uint8_t* pool, uint64_t pool_len, const uint32_t* off, const uint32_t* len, int n,
                         uint32_t* k, int32_t* hcodes, hipStream_t s) {
  if (n > 0) k_hash_scalars<<<nblk(n, 64), 64, 0, s>>>(pool, pool_len, off, len, n, k, hcodes);
}
void launch_hash_points(const uint32_t* k, const int32_t* hcodes, int n, const PointG1* tab, PointG1* out,
                        hipStream_t s) {
  if (n > 0) k_hash_points<<<nblk(n, 4), 64, 0, s>>>(k, hcodes, n, tab, out);
}
void launch_merge_hash_codes(const int32_t* hcodes, int n, int32_t* codes, hipStream_t s) {
  if (n > 0) k_merge_hash_codes<<<nblk(n, 256), 256, 0, s>>>(hcodes, n, codes);
}
void launch_verify_msgs(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int32_t* codes,
                        hipStream_t s) {
  if (n > 0) k_msgs_verify<<<nblk(n, 4), 64, 0, s>>>(in, n, tab, hpts, codes);
}
// false (nothing launched, the codes untouched) above kSig12MaxN, as launch_verify_split
bool launch_verify_msgs_split(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int32_t* codes,
                              uint8_t* ws, hipStream_t s) {
  if (n > kSig12MaxN) return false;
  if (n <= 0) return true;
  Gt* fe = (Gt*)ws;
  k_msgs_miller<<<nblk(n, 4), 64, 0, s>>>(in, n, tab, hpts, fe);
  launch_fe12(fe, n, ws + verify_split_fe_bytes(n), s);
  launch_fe_verdicts(fe, n, codes, s);
  return true;
}
}  // namespace hg
