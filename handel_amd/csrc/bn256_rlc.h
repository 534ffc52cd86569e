// bn256_rlc.h — random linear combination of a batch's aggregate checks
// (hg_verify_aggregate_rlc): the coefficient rule, shared by the
// host and the device, and the launchers of bn256_rlc.hip.
#pragma once
#include "hg_sha256.h"
#if defined(__HIPCC__)
#include "bn256_kernels.h"
#endif

namespace hg {

static constexpr uint32_t kRlcMaxGroup = 4096;
static constexpr int kRlcBits = 64;  // bits of a coefficient: subset products per group
// what every combined call (hg_rlc.cpp, hg_msgs_rlc.cpp, hg_batch_rlc.cpp) accepts as its group size
inline bool rlc_group_ok(uint32_t group) { return group >= 1 && group <= kRlcMaxGroup; }
// groups of a batch of n checks: the last one may be ragged
inline size_t rlc_groups(size_t n, uint32_t group) { return (n + group - 1) / group; }

// the first 8 digest bytes as a little-endian integer (h: the digest's big-endian
// words); 0, which would drop the check from its group, becomes 1
HG_HD uint64_t rlc_coeff_from_digest(uint32_t h0, uint32_t h1) {
  const uint64_t r = (uint64_t)__builtin_bswap32(h0) | ((uint64_t)__builtin_bswap32(h1) << 32);
  return r ? r : 1;
}
// r_i = SHA-256("hg-rlc-v1" || seed || LE64(i)): 49 bytes, one block
HG_HD uint64_t rlc_coeff(const uint8_t seed[32], uint64_t i) {
  uint8_t m[49] = {'h', 'g', '-', 'r', 'l', 'c', '-', 'v', '1'};
  for (int k = 0; k < 32; k++) m[9 + k] = seed[k];
  for (int k = 0; k < 8; k++) m[41 + k] = (uint8_t)(i >> (8 * k));
  uint32_t h[8];
  sha256_words(m, sizeof m, h);
  return rlc_coeff_from_digest(h[0], h[1]);
}

#if defined(__HIPCC__)
struct RlcSeed {
  uint8_t b[32];
};
// by value into launch_rlc_prep; seed == nullptr (a probe brings its coefficients): zeros
inline RlcSeed rlc_seed_of(const uint8_t* seed) {
  RlcSeed sd{};
  for (int k = 0; seed && k < 32; k++) sd.b[k] = seed[k];
  return sd;
}
// a G1 point in Jacobian coordinates between the two G1 kernels
struct RlcJac {
  Fp x, y, z;
};
// counters of one call, read back by the host in one copy
struct RlcHdr {
  uint32_t failed_members;  // live members of the groups that failed: the recheck's size
  uint32_t groups;          // groups with a live member
  uint32_t groups_failed;
  uint32_t non_g2;  // hg_verify_batch_rlc* (bn256_brlc.h): live checks whose key is not a proven member of G2
};
struct Gt;

// r[i] = coeffs ? coeffs[i] : rlc_coeff(seed, i); gcodes[g] = HG_OK; hdr cleared
void launch_rlc_prep(RlcSeed seed, const uint64_t* coeffs, int n, int ngroups, uint64_t* r, int32_t* gcodes,
                     RlcHdr* hdr, hipStream_t s);
// jac[i] = r[i] pts[i] (infinity where codes[i] != HG_OK: the prologue's codes
// will do, the fold only takes checks away)
void launch_rlc_g1_mul(const PointG1* pts, const int32_t* codes, const uint64_t* r, int n, RlcJac* jac, hipStream_t s);
// gpts[g] = the sum of jac[i] over the checks i of group g whose code is HG_OK,
// affine; glive[g] = how many they are
void launch_rlc_g1_sum(const RlcJac* jac, const int32_t* codes, int n, uint32_t group, int ngroups, PointG1* gpts,
                       uint32_t* glive, hipStream_t s);
// P[64 g + b] = the product of x[i] over the live members i of group g with bit
// b of r[i] set (one when there is none), then z[g] = prod x[i]^r[i] by Horner
// over the 64 subset products
void launch_rlc_gt(const Gt* x, const int32_t* codes, const uint64_t* r, int n, uint32_t group, int ngroups, Gt* P,
                   Gt* z, hipStream_t s);
// hdr: groups with a live member, groups whose code is not HG_OK, their live members
void launch_rlc_count(const int32_t* gcodes, const uint32_t* glive, int ngroups, RlcHdr* hdr, hipStream_t s);
// check i is a live member of a group that failed
HG_DEV bool rlc_failed_member(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, int i) {
  return i < n && codes[i] == HG_OK && gcodes[(uint32_t)i / group] != HG_OK;
}
// bcount[b] = the failed groups' live members before block b of 256 checks
// (ceil(n / 256) words): what a gather kernel ranks its members by
void launch_rlc_failed_scan(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, uint32_t* bcount,
                            hipStream_t s);
// The live members of the failed groups, in index order, into compact arrays
// (m = hdr's failed_members entries): idx[j] = the check, csigs its marshal, cy
// its fold value, ccodes[j] = HG_OK. bcount: ceil(n / 256) words of workspace.
void launch_rlc_gather(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, const uint8_t* sigs,
                       const Gt* y, uint32_t* bcount, uint32_t* idx, uint8_t* csigs, Gt* cy, int32_t* ccodes,
                       hipStream_t s);
// codes[idx[j]] = ccodes[j]
void launch_rlc_scatter(const uint32_t* idx, const int32_t* ccodes, int m, int32_t* codes, hipStream_t s);
#endif

}  // namespace hg
