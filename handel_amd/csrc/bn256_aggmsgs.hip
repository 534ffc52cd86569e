// bn256_aggmsgs.hip — aggregate requests that each carry their own message
// (VerifyMultiSignature(msg, ms, reg, cons), crypto.go:120-137, and
// processing.go:342-368 verifySignature, with msg per request): what joins the
// G2 fold (launch_aggregate), the per-message hash (bn256_msgs.hip) and the
// two-pairing check on H per request (k_msgs_verify).
//
//   k_aggmsgs_levels  the level check of processing.go:350-352, before the fold
//   k_aggmsgs_merge   signature decode into the fold's CheckIn records and the
//                     request's code in DESIGN §1's order, after the fold
#include <hip/hip_runtime.h>

#include "bn256_decode.h"

namespace hg {
static inline int nblk(int n, int b) { return (n + b - 1) / b; }

__global__ __launch_bounds__(256) void k_aggmsgs_levels(const AggRequest* reqs, int n, uint32_t nreg, int32_t* lvl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const AggRequest r = reqs[i];
  lvl[i] = level_ok(r, nreg) ? HG_OK : HG_ERR_LEVEL;
}

// One thread per request, after the fold has turned lvl[i] into HG_OK,
// HG_ERR_LEVEL or HG_ERR_EMPTY_AGG and written the aggregate key of every
// request that passed the level check into in[i].pk:
//   signature unmarshal error > HG_ERR_LEVEL > the hash code (HG_ERR_HASH_EOF, or
//   HG_ERR_ARG for a message range outside the pool) > HG_ERR_EMPTY_AGG > HG_OK,
// HG_OK being what k_msgs_verify replaces with the pairing verdict; it reports
// on no other request. The decoded signature goes to in[i].sig whatever the
// code is (the pairing kernel reads every record). A request with a level
// error has no aggregate key: its record is marked as infinity, which marshals
// as zeros, as an empty bitset's does.
__global__ __launch_bounds__(64) void k_aggmsgs_merge(const uint8_t* sigs, int n, int flavor, const int32_t* lvl,
                                                     const int32_t* hcodes, CheckIn* in, int32_t* codes) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  PointG1 S;
  int32_t code = decode_g1_one(sigs + (size_t)i * 64, flavor, S);
  in[i].sig = S;
  const int32_t l = lvl[i];
  if (l == HG_ERR_LEVEL) in[i].pk.inf = 1;
  if (code == HG_OK && l == HG_ERR_LEVEL) code = HG_ERR_LEVEL;
  if (code == HG_OK) code = hcodes[i];
  if (code == HG_OK) code = l;
  codes[i] = code;
}

void launch_aggmsgs_levels(const AggRequest* reqs, int n, uint32_t nreg, int32_t* lvl, hipStream_t s) {
  if (n > 0) k_aggmsgs_levels<<<nblk(n, 256), 256, 0, s>>>(reqs, n, nreg, lvl);
}
void launch_aggmsgs_merge(const uint8_t* sigs, int n, int flavor, const int32_t* lvl, const int32_t* hcodes,
                          CheckIn* in, int32_t* codes, hipStream_t s) {
  if (n > 0) k_aggmsgs_merge<<<nblk(n, 64), 64, 0, s>>>(sigs, n, flavor, lvl, hcodes, in, codes);
}
}  // namespace hg
