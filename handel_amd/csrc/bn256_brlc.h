// bn256_brlc.h — random linear combination of independent checks on arbitrary
// keys (hg_verify_batch_rlc, hg_verify_batch_msgs_rlc): the
// launchers of bn256_batchrlc.hip. The rest of the flow is bn256_mrlc.h's and
// bn256_rlc.h's.
#pragma once
#include "bn256_mrlc.h"
#include "bn256_rlc.h"

namespace hg {

#if defined(__HIPCC__)
// hashedMessage's scalar of one message, by value into a launch
struct BrlcScalar {
  uint32_t w[8];
};
// The one-message form's per-check arrays: k[8 i ..] = k1, hcodes[i] = code
// (HG_OK or HG_ERR_HASH_EOF) and h[i] = *h1 for every check, what
// launch_hash_scalars and launch_hash_points leave when every check carries
// the same message.
void launch_brlc_one_message(BrlcScalar k1, const PointG1* h1, int32_t code, int n, uint32_t* k, int32_t* hcodes,
                             PointG1* h, hipStream_t s);
// launch_mrlc_miller with the G2 membership verdict of the check's key out of
// the loop's end point (the rule of DESIGN §3n): member[i] = 1 for a key at
// infinity or a key proven in G2, else 0; f[i] of a check with member[i] = 0 is
// one, so that no zero enters the group's product. hstride: 1 for check i on
// hpts[i], 0 for every check on hpts[0].
void launch_brlc_miller(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int hstride, Gt* f,
                        uint32_t* member, hipStream_t s);
// A group that holds a check with codes[i] == HG_OK and member[i] == 0 fails:
// gcodes[g] = HG_ERR_SIG_INVALID, and hdr->non_g2 += the number of such checks.
void launch_brlc_members(const int32_t* codes, const uint32_t* member, int n, uint32_t group, int ngroups,
                         int32_t* gcodes, RlcHdr* hdr, hipStream_t s);
// hg_debug_g2_member: out[i] = (pks[i], the infinity signature), the key at
// infinity where codes[i] != HG_OK; *gen = the G1 generator
void launch_brlc_probe_checks(const PointG2* pks, const int32_t* codes, int n, CheckIn* out, PointG1* gen,
                              hipStream_t s);
#endif

}  // namespace hg
