// bn256_xprobew2.hip — hg_debug_xinst's form 1: the layout-S instances on
// 16-lane teams spread over 2 waves (make_team_split), as k_verify_sig_split<2>
// runs them (bn256_sigw2.hip). Like that unit, this one alone builds the
// split branches of bn256_xprog.h (HG_TEAM_SPLIT before any include).
#define HG_TEAM_SPLIT 2
#include "bn256_xprobe_kernel.h"

namespace hg {

// the caller has checked that inst is a layout-S instance (bn256_xprobe.hip)
void launch_xprobe_w2(int inst, const uint32_t* in, int n, uint32_t* out, hipStream_t s) {
  if (n <= 0) return;
  switch (kXProbeInfo[inst].group) {
#define HG_XPROBE_CASE(G) \
  case G: launch_xprobe_group<G>(inst, in, n, out, s); break;
    HG_XPROBE_S_GROUPS(HG_XPROBE_CASE)
#undef HG_XPROBE_CASE
    default: break;
  }
}

}  // namespace hg
