// bn256_mrlc.h — random linear combination of aggregate checks that each carry
// their own message (hg_verify_aggregate_msgs_rlc): the scaling
// of hashedMessage's scalar by a coefficient, shared by the host and the
// device, and the launchers of bn256_msgsrlc.hip.
#pragma once
#include "hg_sha256.h"
#if defined(__HIPCC__)
#include "bn256_kernels.h"
#endif

namespace hg {

// hi 2^256 + a < 2 Order (a: 8 little-endian words, hi: 0 or 1) -> that value mod Order
HG_HD void ord_csub(uint32_t a[8], uint32_t hi) {
  const uint32_t order[8] = {HG_ORDER32};
  uint32_t d[8], br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a[i] - order[i] - br;
    d[i] = (uint32_t)t;
    br = (uint32_t)(t >> 63);
  }
  const bool sub = hi != 0 || br == 0;  // the value is at least Order
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = sub ? d[i] : a[i];
}

// out = r k mod Order: the 64 x 256-bit product by Horner's rule over the bits
// of r, reduced at every step. Order has 256 bits, so a doubled or summed
// residue (< 2 Order) may carry out of the eight words: the carry goes into the
// conditional subtraction. Any 256-bit k is served (2^256 < 2 Order: one
// subtraction reduces it first); hashedMessage's scalars are already below Order.
HG_HD void mrlc_scale(uint32_t out[8], uint64_t r, const uint32_t k[8]) {
  uint32_t kk[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    kk[i] = k[i];
    acc[i] = 0;
  }
  ord_csub(kk, 0);
  for (int bit = 63; bit >= 0; bit--) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {  // acc = 2 acc
      const uint32_t v = acc[i];
      acc[i] = (v << 1) | c;
      c = v >> 31;
    }
    ord_csub(acc, c);
    const uint32_t m = 0u - (uint32_t)((r >> bit) & 1);
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {  // acc += k where the bit is set
      carry += (uint64_t)acc[i] + (kk[i] & m);
      acc[i] = (uint32_t)carry;
      carry >>= 32;
    }
    ord_csub(acc, (uint32_t)carry);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = acc[i];
}

#if defined(__HIPCC__)
struct Gt;

// rk[8 i ..] = r[i] k[8 i ..] mod Order where hcodes[i] is HG_OK, else zeros
// (launch_hash_points does not read the scalar of such a message)
void launch_mrlc_scalars(const uint32_t* k, const int32_t* hcodes, const uint64_t* r, int n, uint32_t* rk,
                         hipStream_t s);
// pts[i] = in[i].sig
void launch_mrlc_sigs(const CheckIn* in, int n, PointG1* pts, hipStream_t s);
// The scaled check records: out[i].pk = in[i].pk where codes[i] is HG_OK, else
// infinity; out[i].sig = gpts[g] for the first member of group g whose code is
// HG_OK, infinity for every other member. carrier: ngroups words of workspace.
void launch_mrlc_checks(const CheckIn* in, const int32_t* codes, const PointG1* gpts, int n, uint32_t group,
                        int ngroups, uint32_t* carrier, CheckIn* out, hipStream_t s);
// f[i] = the Miller value of check i on hpts[i] (launch_verify_msgs_split's first half)
void launch_mrlc_miller(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, Gt* f, hipStream_t s);
// z[g] = the product of f[i] over the members i of group g whose code is HG_OK (one when there is none)
void launch_mrlc_product(const Gt* f, const int32_t* codes, int n, uint32_t group, int ngroups, Gt* z,
                         hipStream_t s);
// The members of the failed groups whose code is HG_OK, in index order, into
// compact arrays (m = RlcHdr's failed_members entries): idx[j] = the request,
// cchecks[j] and ch[j] its check record and its H, ccodes[j] = HG_OK. bcount:
// ceil(n / 256) words of workspace.
void launch_mrlc_gather(const int32_t* codes, const int32_t* gcodes, int n, uint32_t group, const CheckIn* in,
                        const PointG1* h, uint32_t* bcount, uint32_t* idx, CheckIn* cchecks, PointG1* ch,
                        int32_t* ccodes, hipStream_t s);
#endif

}  // namespace hg
