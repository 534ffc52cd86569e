// bn256_xprobe.hip — hg_debug_xinst's kernels on one-wave teams (form 0): every
// bound instance of bn256_xtab.h, one kernel per group of bn256_xprobe.h. The
// split-team form of the layout-S instances (form 1) is bn256_xprobew2.hip.
#include "bn256_xprobe_kernel.h"

namespace hg {

void launch_xprobe_w2(int inst, const uint32_t* in, int n, uint32_t* out, hipStream_t s);  // bn256_xprobew2.hip

int xprobe_instances() { return kXProbeInstances; }

// the entry of kXProbeInfo for probe instance inst: the numbered cases, then
// the extra ones from kXProbeExtraBase on; -1: no such instance
static int xprobe_entry(int inst) {
  if (inst >= 0 && inst < kXProbeInstances) return inst;
  if (inst >= kXProbeExtraBase && inst < kXProbeExtraBase + kXProbeExtra) return kXProbeInstances + inst - kXProbeExtraBase;
  return -1;
}

// the team region of instance inst in form `form`: its elements, or 0 when
// there is no such instance or the instance's layout has no such form
int xprobe_region_elems(int inst, int form) {
  const int e = xprobe_entry(inst);
  if (e < 0 || form < 0 || form > 1) return 0;
  if (form == 1 && kXProbeInfo[e].layout != XPL_S) return 0;
  return kXProbeInfo[e].elems;
}

// the caller has checked (inst, form) with xprobe_region_elems
void launch_xprobe(int inst, int form, const uint32_t* in, int n, uint32_t* out, hipStream_t s) {
  if (n <= 0) return;
  const int e = xprobe_entry(inst);
  if (form == 1) {
    launch_xprobe_w2(e, in, n, out, s);
    return;
  }
  switch (kXProbeInfo[e].group) {
#define HG_XPROBE_CASE(G) \
  case G: launch_xprobe_group<G>(e, in, n, out, s); break;
    HG_XPROBE_GROUPS(HG_XPROBE_CASE)
#undef HG_XPROBE_CASE
    default: break;
  }
}

}  // namespace hg
