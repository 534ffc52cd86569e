// bn256_redq.h — the reduction tail of rounds with R-shifted linear terms, in
// ONE carry chain (the 12-lane pairing programs' rounds, bn256_xprog.h).
//
// After the REDC digits, columns 11..20 of the accumulator hold
//     V = sum_j c_j 2^(26 j)  <  (QMAX + 1) p          (c_j: 64-bit columns)
// with QMAX the round's own bound from the generator (tools/
// gen_g2_schedule.py check_xround). acc_reduce_wide normalises the columns,
// divides the top limb and then walks the ten limbs a second time to subtract
// q p. Here q comes from the top two columns BEFORE the chain,
//     t = c_9 + floor(c_8 / 2^26),   q = floor(t / (p_9 + 1)),
// and -q p rides along the normalising chain as q (Z_j - p_j), where
//     Z = {2^26, 2^26 - 1 (x 8), -1}
// is zero re-spread over the limbs: every low-limb addend is non-negative, so
// the chain stays unsigned (one v_mad_u64_u32 per limb), and the top limb takes
// -q (p_9 + 1) in 32-bit arithmetic.
//
// Range: t 2^234 <= V < (t + 1 + D) 2^234 with D = ceil(2 max c_j / 2^52) (the
// columns below c_8), and t - p_9 <= q (p_9 + 1) <= t, so
//     0 <= V - q p < (p_9 + 1 + D + q) 2^234  <  2p   (generator-checked):
// the lazy form's result as it stands, and barely above p when it is not below
// it — so the canonical form subtracts p under the exact top-limb test of
// fp_csub_rare instead of a ten-limb borrow chain and ten selects.
//
// Plain C++ on purpose: the same functions compile for the host (tests/native/
// reduce_wide_host.cpp) and for the device.
#pragma once
#include <stdint.h>

#include "bn256_constants.h"

#if defined(__HIPCC__)
#define HG_HD __host__ __device__ __forceinline__
#else
#define HG_HD inline
#endif

namespace hg {

// the largest per-round bound the one-chain forms take (gen_g2_schedule.py
// ONE_CHAIN_QMAX_LIMIT): (QMAX + 1) (p_9 + 1) stays far inside 32 bits
static constexpr int kRedqMaxQ = 64;
// up to here q is a sum of compares; above, one division by a constant
static constexpr int kRedqCompareQ = 2;

// d = p_9 + 1 and floor(t / d) = (t M) >> 53 with M = floor(2^53 / d) + 1: exact
// while t (M d - 2^53) < 2^53, that is for every t < 2^31 (M d - 2^53 <= d < 2^22)
static constexpr uint32_t kRedqPLimbs[10] = {HG_PLIMBS};
static constexpr uint32_t kRedqD = kRedqPLimbs[9] + 1u;
static constexpr uint32_t kRedqM = (uint32_t)((1ull << 53) / kRedqD) + 1u;
static_assert(kRedqD > (1u << 21) && (uint64_t)(kRedqMaxQ + 2) * kRedqD + (1u << 14) < (1ull << 31), "t below 2^31");

HG_HD uint32_t redq_p_limb(int j) {
  const uint32_t pl[10] = {HG_PLIMBS};
  return pl[j];
}
// Z_j - p_j for the low limbs
HG_HD uint32_t redq_np_limb(int j) {
  return (j == 0 ? (1u << 26) : kMask) - redq_p_limb(j);
}

// r = V - q p as ten limbs (nine of 26 bits, the top one whole), in [0, 2p);
// LAZY = false: the canonical element V mod p.
// c: the accumulator's columns 11..20.
template <int QMAX, bool LAZY>
HG_HD void redq_tail(uint32_t (&r)[10], const uint64_t* c) {
  static_assert(QMAX >= 1 && QMAX <= kRedqMaxQ, "the generator's per-round quotient bound");
  constexpr uint32_t d = kRedqD;
  const uint32_t t = (uint32_t)c[9] + (uint32_t)(c[8] >> 26);
  uint32_t q = 0;
  if (QMAX <= kRedqCompareQ) {
#pragma unroll
    for (int k = 1; k <= QMAX; k++) q += t >= (uint32_t)k * d ? 1u : 0u;
  } else {
    q = (uint32_t)(((uint64_t)t * kRedqM) >> 53);  // t / d: one v_mul_hi_u32 and a shift
  }
  uint64_t carry = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const uint64_t v = c[j] + (uint64_t)q * redq_np_limb(j) + carry;
    r[j] = (uint32_t)v & kMask;
    carry = v >> 26;
  }
  r[9] = (uint32_t)(c[9] + carry) - q * d;
  if (!LAZY) {
    // r >= p implies r_9 >= p_9: about one lane in 2^15 (see above)
    if (__builtin_expect(r[9] >= redq_p_limb(9), 0)) {
      uint32_t s[10];
      int32_t br = 0;
#pragma unroll
      for (int i = 0; i < 10; i++) {
        const int32_t v = (int32_t)r[i] - (int32_t)redq_p_limb(i) - br;
        br = (v >> 31) & 1;
        s[i] = (uint32_t)v & kMask;
      }
      if (br == 0) {
#pragma unroll
        for (int i = 0; i < 10; i++) r[i] = s[i];
      }
    }
  }
}

}  // namespace hg
